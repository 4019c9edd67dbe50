"""The three device decoders' host halves under random input (no device is needed): on the corpus of the generator kits
(tests/charstring_fuzz_kit.py, tests/gvar_fuzz_kit.py) over a fixed list of seeds,

  - the host reader is the kit's interpreter / restatement bit for bit (charstrings: `CFF ` and CFF2, the latter at the default
    position and placed at two others; gvar: outlines and the advance deltas of rule G7 at three positions per face);
  - fontTools, which shares no line with either, draws the same glyphs: equal where no f32 rounding on the way to a coordinate
    changed a value, else within the bound the kit derives for that coordinate — the number of such roundings x half an ulp of the
    largest magnitude on the way (fontTools works in f64 from the same operands).  Glyphs that fail by the rules are left out, and
    the few constructs fontTools itself cannot read (the kits name them);
  - the corpus reaches every feature the kits list, each on at least three glyphs of different faces, counted from what the
    interpreters met and not from what the generator meant;
  - at least 70 % of the glyphs deliver a command, at most 25 % fail by rule, at most 10 % are empty;
  - every deliberately wrong variant of the interpreters disagrees with the host reader on some glyph of the corpus."""
import numpy as np
import pytest

pytest.importorskip("fontTools")

import charstring_edge_programs as K  # noqa: E402
import charstring_fuzz_kit as F  # noqa: E402
import gvar_fuzz_kit as GF  # noqa: E402
import gvar_instances_kit as G  # noqa: E402
import phantom_advances_kit as P  # noqa: E402

DECODERS = ("cff", "cff2")


@pytest.fixture(scope="module")
def charstrings(vg):
    """{decoder: [(face, font bytes, {position: (description, host table)}, [(outcome, features) per glyph id at the default])]}"""
    out = {}
    for key in DECODERS:
        cff2 = key == "cff2"
        out[key] = []
        for seed in F.SEEDS:
            face = F.face(seed, cff2)
            font = face.font()
            views = {c if c is None else tuple(c): F.host_views(vg, font, cff2, c) for c in (F.POSITIONS2 if cff2 else (None,))}
            d = views[None][0]
            out[key].append((face, font, views, [F.features(d, g, cff2) for g in range(len(face.glyphs))]))
    return out


@pytest.fixture(scope="module")
def gvars(vg):
    """[(face, {position: (description, host table, host advance deltas)})]"""
    out = []
    for seed in GF.SEEDS:
        f = GF.face(seed)
        out.append((f, {tuple(c): GF.host_views(vg, f, c) for c in f.positions}))
    return out


@pytest.mark.parametrize("key", DECODERS)
def test_the_host_reader_is_the_interpreter_on_every_glyph(charstrings, key):
    n = 0
    for face, font, views, _ in charstrings[key]:
        want = face.desc()
        for position, (d, host) in views.items():
            if position is None:
                for k, v in want.items():          # the host's description is the one the kit builds directly
                    assert (d[k] is None) if v is None else np.array_equal(d[k], v), (face.name, k)
            assert F.first_difference(f"{face.name} at {position}", d, host, key == "cff2") is None
            n += len(face.glyphs)
    assert n == len(F.SEEDS) * F.N_GLYPHS * (3 if key == "cff2" else 1)


def test_the_host_reader_is_the_restatement_on_every_gvar_face(gvars):
    for f, views in gvars:
        for coords, (_, host, advances) in views.items():
            assert GF.first_difference(f, coords, host, advances) is None
    assert {f.n_axes for f, _ in gvars} == {1, 2, 3}


def _compare(name, tracked, other, state):
    """the Tracked coordinates of one glyph against another reader's floats"""
    assert len(tracked) == len(other), name
    for a, b in zip(tracked, other):
        dev, bound = abs(float(a) - b), a.bound() * (1 + 2.0 ** -20)      # (the other reader's own f64 roundings)
        assert dev <= bound, (name, float(a), b, a.n, bound)
        state["exact" if a.n == 0 else "rounded"] += 1
        if dev > state["worst"][0]:
            state["worst"] = (dev, bound, name)


@pytest.mark.parametrize("key", DECODERS)
def test_fonttools_draws_what_the_host_reader_delivers(charstrings, key):
    cff2 = key == "cff2"
    state = {"exact": 0, "rounded": 0, "worst": (0.0, 0.0, ""), "glyphs": 0, "left_out": 0}
    for face, font, views, runs in charstrings[key]:
        for position, (d, host) in views.items():
            if position == tuple(F.POSITIONS2[1]):               # (exact factors: the default position's case again)
                continue
            drawn = F.fonttools_commands(font, None if not cff2 else {"wght": 0.0 if position is None else position[0] / 16384.0}, normalized=True)
            for g in range(len(face.glyphs)):
                o, reached = runs[g]
                if o.end == "fail" or reached & set(F.FONTTOOLS_BLIND):
                    state["left_out"] += 1
                    continue
                t = F.tracked_run(d, g, cff2)
                assert K.glyph_commands(host, g) == F.commands_of(t)           # (the same values, tracked)
                name = f"{face.name} at {position}, glyph id {g}"
                assert drawn[g] is not None, name
                kinds, floats = drawn[g]
                # (fontTools closes the last contour where the stream ends without endchar, and in CFF2 always)
                strip = lambda k: k[:-1] if k and k[-1] == K.Z else k  # noqa: E731
                assert strip(list(t.kinds)) == strip(kinds), name
                _compare(name, t.coords, floats, state)
                state["glyphs"] += 1
    dev, bound, name = state["worst"]
    print(f"{key}: {state['glyphs']} glyphs drawn by fontTools ({state['left_out']} left out), {state['exact']} coordinates equal, "
          f"{state['rounded']} rounded; largest deviation {dev!r} font units (its bound {bound!r}) in {name}")
    assert state["glyphs"] >= 0.6 * (state["glyphs"] + state["left_out"]) and state["exact"] > 10000 and state["rounded"] > 1000


def test_fonttools_places_the_points_the_host_reader_delivers(gvars):
    state = {"exact": 0, "rounded": 0, "worst": (0.0, 0.0, ""), "glyphs": 0, "left_out": 0}
    for f, views in gvars:
        for coords, (_, host, _) in views.items():
            tracked = GF.tracked_restate(f.font, coords)
            drawn = GF.fonttools_flat(f.font_for_fonttools, coords)
            for g, t in enumerate(tracked):
                if g in f.blind or g not in drawn:                  # (glyph id 0 has no code point)
                    state["left_out"] += 1
                    continue
                name = f"{f.name} at {list(coords)}, glyph id {g}"
                a, b = int(host["cmd_off"][g]), int(host["cmd_off"][g + 1])
                assert host["kinds"][a:b].tolist() == drawn[g][0], name
                assert np.array([float(v) for v in t], np.float32).tobytes() == host["coords"][host["dat_off"][g]:host["dat_off"][g + 1]].tobytes()
                _compare(name, t, drawn[g][1], state)
                state["glyphs"] += 1
    dev, bound, name = state["worst"]
    print(f"gvar: {state['glyphs']} glyphs placed by fontTools ({state['left_out']} left out), {state['exact']} coordinates equal, "
          f"{state['rounded']} rounded; largest deviation {dev!r} font units (its bound {bound!r}) in {name}")
    assert state["glyphs"] >= 0.6 * (state["glyphs"] + state["left_out"]) and state["exact"] > 10000 and state["rounded"] > 1000


def test_the_corpus_reaches_every_feature_on_three_faces(charstrings, gvars):
    missing = []
    for key in DECODERS:
        faces_of = {}
        for i, (_, _, _, runs) in enumerate(charstrings[key]):
            for _, reached in runs:
                for name in reached:
                    faces_of.setdefault(name, set()).add(i)
        missing += [(key, name, len(faces_of.get(name, ()))) for name in F.FEATURES[key] if len(faces_of.get(name, ())) < 3]
    faces_of = {}
    for i, (f, views) in enumerate(gvars):
        for coords in views:
            for name in GF.features(f, coords):
                faces_of.setdefault(name, set()).add(i)
    missing += [("gvar", name, len(faces_of.get(name, ()))) for name in GF.FEATURES if len(faces_of.get(name, ())) < 3]
    assert not missing, missing


@pytest.mark.parametrize("key", DECODERS)
def test_the_shares_of_the_corpus(charstrings, key):
    n = deliver = fail = empty = 0
    for face, _, _, runs in charstrings[key]:
        for (_, cs), (o, _) in zip(face.glyphs, runs):
            n += 1
            deliver += bool(o.kinds)
            fail += o.end == "fail"
            empty += len(cs) == 0
    print(f"{key}: {n} glyphs, {deliver / n:.1%} deliver a command, {fail / n:.1%} fail by rule, {empty / n:.1%} are empty")
    assert deliver >= 0.70 * n and fail <= 0.25 * n and empty <= 0.10 * n
    # the wave of 63 empty charstrings around one long one
    waves = [[len(cs) for _, cs in face.glyphs[64:128]] for face, _, _, _ in charstrings[key]]
    assert any(sorted(w)[:63] == [0] * 63 and max(w) > 500 for w in waves)


def test_the_shares_of_the_gvar_corpus(gvars):
    n = deliver = empty = 0
    for f, views in gvars:
        host = next(iter(views.values()))[1]
        counts = np.diff(host["cmd_off"].astype(np.int64))
        n += len(counts)
        deliver += int((counts > 0).sum())
        empty += sum(G._Tables(f.font).glyph(g) is None for g in range(len(counts)))
    print(f"gvar: {n} glyphs, {deliver / n:.1%} deliver a command, {empty / n:.1%} are empty")
    assert deliver >= 0.70 * n and empty <= 0.10 * n        # (no gvar glyph fails by rule: only well-formed data is written)


def test_every_wrong_variant_is_caught(charstrings, gvars):
    assert len(F.MUTANTS) + len(GF.MUTANTS) >= 12 and {d for _, d, _ in F.MUTANTS} == set(DECODERS)
    survivors = []
    for rule, key, interpret in F.MUTANTS:
        cff2 = key == "cff2"
        if not any(F.first_difference(face.name, d, host, cff2, interpret) for face, _, views, _ in charstrings[key] for d, host in views.values()):
            survivors.append((key, rule))
    for rule, kind, restate in GF.MUTANTS:
        swap = {"restate": restate} if kind == "outline" else {"restate_deltas": restate}
        if not any(GF.first_difference(f, c, host, adv, **swap) for f, views in gvars for c, (_, host, adv) in views.items()):
            survivors.append(("gvar", rule))
    assert not survivors, survivors


def test_the_sums_of_rule_g7_are_the_restatements_on_the_corpus(gvars):
    """(the advances themselves, through Face::hor_advances: hmtx + the rounded delta)"""
    moved = 0
    for f, views in gvars:
        for coords, (_, _, (d, state)) in views.items():
            assert set(state.tolist()) <= {P.NONE, P.DELTA}
            moved += int(np.count_nonzero(d))
    assert moved > 100
