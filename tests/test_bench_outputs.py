"""`bench.py --dump-outputs DIR`: what the timed step computed, as float32 .npy files of at most 64 MB, the same from run to run.
CPU-only: the SDF bytes are stand-ins; the batches are the benchmark's own (host stage and synthetic generator)."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test_outputs", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.load_product()   # (registers versatiles_glyphs_rs_amd for the imports below)
    return mod


def _size(d):
    return sum(p.stat().st_size for p in Path(d).iterdir())


def test_small_output_is_written_whole(bench, tmp_path):
    from versatiles_glyphs_rs_amd import synthetic as S
    b = S.make_batch(0, 16)
    got = np.random.default_rng(3).integers(0, 256, b.out_bytes, dtype=np.uint8)
    bench.dump_outputs(tmp_path / "out", b, got)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["sdf.npy"]
    sdf = np.load(tmp_path / "out" / "sdf.npy")
    assert sdf.dtype == np.float32 and (sdf == got).all()


def test_large_output_is_a_fixed_sample_of_whole_glyphs_within_the_limit(bench, tmp_path):
    from versatiles_glyphs_rs_amd import synthetic as S
    b = S.make_batch(0, bench.SYNTHETIC_PER_RANK)          # 8192 glyphs of 70x70: 160 MB as float32
    got = np.random.default_rng(4).integers(0, 256, b.out_bytes, dtype=np.uint8)
    bench.dump_outputs(tmp_path / "a", b, got)
    bench.dump_outputs(tmp_path / "b", b, got)
    assert _size(tmp_path / "a") <= bench.DUMP_LIMIT
    sdf, ix = np.load(tmp_path / "a" / "sdf.npy"), np.load(tmp_path / "a" / "sdf_glyph_index.npy")
    assert sdf.dtype == np.float32 and ix.dtype == np.float64 and len(ix) > 1000
    assert (np.diff(ix) > 0).all() and ix[-1] < b.n_glyphs
    off = b.out_off.astype(np.int64)
    assert (sdf == np.concatenate([got[off[g]:off[g + 1]] for g in ix.astype(np.int64)])).all()
    assert (np.load(tmp_path / "b" / "sdf_glyph_index.npy") == ix).all()   # the same sample every run


def test_last_resort_processes_leave_the_outputs_to_the_first(bench, monkeypatch):
    import subprocess
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("VG_SHARE_GPU", raising=False)
    monkeypatch.delenv("VG_DIST_BACKEND", raising=False)
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: subprocess.CompletedProcess(
        cmd, 0 if "-c" in cmd else 1, stdout="2\n" if "-c" in cmd else "", stderr=""))
    started = []

    class FakeProc:
        def __init__(self, cmd, **kw):
            started.append(cmd)

        def communicate(self, timeout=None):
            return '{"value": 1.0, "mpixel_sdf_per_s": 1.0, "ms_per_step": 0.1, "n_gpus": 1}\n', None
    monkeypatch.setattr(subprocess, "Popen", FakeProc)
    bench.launch_ranks(2, ["--gpus", "2", "--dump-outputs", "d", "--steps", "5"])
    assert started[0][started[0].index("--dump-outputs") + 1] == "d"
    assert "--dump-outputs" not in started[1] and "d" not in started[1] and "--steps" in started[1]
