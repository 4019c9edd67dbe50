"""GPU: what the raw v_sqrt_f32 returns, as far as the span kernel's exactness argument uses it ("The three
square roots").  The kernel takes `__builtin_amdgcn_sqrtf` for phase 1's U, for the group radius and for the decide step's sq;
the argument needs two facts about the instruction, both over EVERY non-negative finite f32 input:

  * on normal inputs the result is within 1 ulp of the correctly rounded root (the documented accuracy of the instruction);
    INFL = 1 + 2^-9, the 1.001 of h(F) and the 3e-4 of dl are sized against that figure;
  * a denormal input returns exactly 0 (and so does +0): U and r_g then fall back on their absolute pad, and the decide step
    gets sq = 0, hence dl = inf, hence an undecided pixel, which is evaluated exactly.

tools/ubench/sqrt_probe.hip compares the instruction with `__builtin_sqrtf` on all 2^31 - 2^23 bit patterns (well under a second);
it is built here with the product's floating-point flags, as tests/test_charstring2_table_sanitized.py builds its program, and
run once.  profiles/sweep_isa_ab.txt holds the output recorded with the change."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_raw_sqrt_is_within_one_ulp_and_flushes_denormals(tmp_path):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path / "sqrt_probe"
    built = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fno-fast-math",
                            str(ROOT / "tools" / "ubench" / "sqrt_probe.hip"), "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-2000:]
    m = re.search(r"^RESULT max_ulp=(\d+) differ=(\d+) den_zero=(\d+) den_max_ulp=(\d+) zero_bits=0x([0-9A-Fa-f]{8})$", run.stdout, re.M)
    assert m, run.stdout[-1000:]
    max_ulp, differ, den_zero, den_max_ulp, zero_bits = int(m[1]), int(m[2]), int(m[3]), int(m[4]), int(m[5], 16)
    assert max_ulp <= 1                       # normal inputs: at most 1 ulp from the correctly rounded root
    assert 0 < differ                         # (the probe compares two different things: the raw instruction is not the rounded root)
    assert den_zero == (1 << 23) - 1          # every denormal input returns exactly 0 ...
    assert den_max_ulp == 0                   # ... (so there are no other denormal results to be off)
    assert zero_bits == 0                     # sqrt(+0) = +0
