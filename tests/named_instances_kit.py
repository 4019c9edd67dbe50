"""Variable files WITH NAMED INSTANCES for the tests of vg_manager_add_font_named_instances, and a strict restatement of the rule
that gives an instance its font id.  No tests here.

The files are those of tests/gvar_instances_kit.py (the 315-glyph `glyf` + `gvar` fixtures, a hand-written face) with instance
records added to their `fvar` by fontTools: records with and without a postScriptNameID (in one table, and a table whose records
have no room for one), two records that arrive at one font id, a record whose subfamily name id `name` does not have, with and
without a variations PostScript name prefix (name id 25).

`instance_ids` restates include/vgfont.h's rule from what fontTools reads of `fvar` and `name`: which PostScript name an instance
goes by.  From there on an instance's id comes as every file's does — parse_font_name(family, ps_name) (the reference's parser,
held against it by tests/test_ingestion_and_sinks.py), metadata.rs' generate_name (restated here) and name_to_id."""
import io

import gvar_instances_kit as G

NO_NAME = 0xFFFF
ABSENT_NAME_ID = 999      # no record of `name` has it

# (subfamily: a string (a name record is added for it) or a raw name id; ps: None (0xFFFF), a string, or a raw name id; location)
ONE_AXIS = [dict(subfamily="Medium", ps=None, location={"wght": 525}),
            dict(subfamily="Semi Bold", ps="SynthGvarRoman-SemiBold", location={"wght": 650}),
            dict(subfamily="Black", ps=None, location={"wght": 900}),
            dict(subfamily="Heavy Black", ps="SynthGvar-Black", location={"wght": 880}),       # the id of the record before it
            dict(subfamily=ABSENT_NAME_ID, ps=None, location={"wght": 700}),                    # "<prefix>-"
            dict(subfamily="Regular", ps=ABSENT_NAME_ID, location={"wght": 400})]               # a postScriptNameID `name` lacks
TWO_AXES = [dict(subfamily="Medium", ps=None, location={"wght": 650, "wdth": 100}),
            dict(subfamily="Extended Bold", ps=None, location={"wght": 775, "wdth": 150}),
            dict(subfamily="Extended Black", ps=None, location={"wght": 900, "wdth": 200})]
EDGE = [dict(subfamily="Light", ps=None, location={"wght": 0.5}), dict(subfamily="Bold", ps=None, location={"wght": 1.0}),
        dict(subfamily="Thin", ps=None, location={"wght": -0.5}), dict(subfamily="Regular", ps=None, location={"wght": 0.0})]

_CACHE = {}


def with_instances(font_bytes, records, prefix=None, room_for_ps=True):
    """the font with `records` as the instance records of its fvar.  prefix: the string of name id 25 (None: no such record).
    room_for_ps False: every record's ps must be None, and the records are written without the postScriptNameID field"""
    from fontTools.ttLib import TTFont
    from fontTools.ttLib.tables._f_v_a_r import NamedInstance
    f = TTFont(io.BytesIO(font_bytes), recalcBBoxes=False, recalcTimestamp=False)
    name, fvar = f["name"], f["fvar"]
    if prefix is not None:
        name.setName(prefix, 25, 3, 1, 0x409)
    fvar.instances = []
    for r in records:
        inst = NamedInstance()
        inst.subfamilyNameID = r["subfamily"] if isinstance(r["subfamily"], int) else name.addName(r["subfamily"], platforms=((3, 1, 0x409),))
        ps = r["ps"]
        inst.postscriptNameID = NO_NAME if ps is None else ps if isinstance(ps, int) else name.addName(ps, platforms=((3, 1, 0x409),))
        inst.coordinates = {a.axisTag: float(r["location"].get(a.axisTag, a.defaultValue)) for a in fvar.axes}
        fvar.instances.append(inst)
    if not room_for_ps:
        assert all(r["ps"] is None for r in records)     # (fontTools then leaves the field out of every record)
    else:
        assert any(r["ps"] is not None for r in records) or not records
    out = io.BytesIO()
    f.save(out)
    return out.getvalue()


def files():
    """name -> (font bytes, records): built once"""
    if not _CACHE:
        _CACHE["shear"] = (with_instances(G.variable_glyf_fira("shear"), ONE_AXIS), ONE_AXIS)
        _CACHE["scale_prefix"] = (with_instances(G.variable_glyf_fira("scale"), ONE_AXIS, prefix="SynthVF"), ONE_AXIS)
        _CACHE["two_axes_no_room"] = (with_instances(G.variable_glyf_fira("two_axes"), TWO_AXES, room_for_ps=False), TWO_AXES)
        _CACHE["edge"] = (with_instances(G.edge_faces()["inference"][0], EDGE, room_for_ps=False), EDGE)
    return _CACHE


def no_instances(font_bytes):
    return with_instances(font_bytes, [])


# ---- the restatement ---------------------------------------------------------------------------------------------------------

WEIGHTS = {100: "Thin", 200: "ExtraLight", 300: "Light", 400: "Regular", 500: "Medium", 600: "SemiBold", 700: "Bold", 800: "ExtraBold",
           900: "Black"}


def generate_name(family, style, weight, width):
    """FontMetadata::generate_name (metadata.rs): family [width] weight [style]"""
    parts = [family] + ([width] if width != "normal" else []) + [WEIGHTS.get(weight, "Unknown")] + ([style] if style != "normal" else [])
    return " ".join(parts)


def _names(f):
    """name id -> string: a later record of an id replaces an earlier one (metadata.rs' HashMap over the records)"""
    out = {}
    for rec in f["name"].names:
        out[rec.nameID] = rec.toUnicode()
    return out


def ps_names(font_bytes):
    """(family, [the PostScript name of every instance record]) by the rule, from fontTools' reading"""
    from fontTools.ttLib import TTFont
    f = TTFont(io.BytesIO(font_bytes))
    names = _names(f)
    family = names.get(1, "")
    prefix = names.get(25, "") or "".join(c for c in family if c.isascii() and c.isalnum())
    out = []
    for inst in f["fvar"].instances:
        ps_id = getattr(inst, "postscriptNameID", NO_NAME)
        if ps_id != NO_NAME and ps_id in names:
            out.append(names[ps_id])
        else:
            out.append(prefix + "-" + names.get(inst.subfamilyNameID, "").replace(" ", ""))
    return family, out


def instance_names(vg, font_bytes):
    """the generated font name of every instance record, in the table's order"""
    family, names = ps_names(font_bytes)
    return [generate_name(*vg.parse_font_name(family, ps)) for ps in names]


def instance_ids(vg, font_bytes):
    """the font id of every instance record, in the table's order"""
    return [vg.name_to_id(name) for name in instance_names(vg, font_bytes)]
