"""What the tests of the batched family tables share (vgsdf_families_create_tables, vgsdf_gvar_advance_deltas_batch and the façade's
vg_manager_set_family_tables_batched): ONE file at N positions, its stores, its descriptions and the host reader's entries per
position.  No tests here.

The yardsticks are the host reader — mgr.font_gvar_advance_deltas for the phantom pass, mgr.family_desc for the entries — and
vgsdf_family_create over those entries; never the batched call itself.  Built on tests/phantom_advances_kit.py,
tests/gvar_instances_kit.py, tests/variable_instances_kit.py and tests/named_instances_kit.py."""
import numpy as np

import gvar_instances_kit as G
import named_instances_kit as NI
import phantom_advances_kit as P
import variable_instances_kit as V

E_ARG, E_GLYF = -1, -4
ARRAYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x", "cmd_pre", "leaf_pre", "pbf_fix")
ENTRY_KEYS = ("code_point", "font_of", "glyph_id", "advance", "scale", "shift_x")
# nine positions of a one-axis file, all different
NINE = ([0], [16384], [8192], [-8192], [5000], [12000], [3000], [-3000], [16000])


def positions_with_a_twin(n):
    """n positions of NINE of which (from n = 3 on) the last repeats the first"""
    out = [list(p) for p in NINE[:n]]
    if n >= 3:
        out[-1] = list(out[0])
    return out


class Placed:
    """ONE file at `positions`: a manager that holds a font id per position (each of the one file: the manager owns the bytes the
    descriptions point into), the device fonts and what the batched call and its yardsticks take.  device_stores: the command
    stores come from vgsdf_fonts_create_gvar (a `glyf` file; held to the host's by tests/test_gpu_gvar_batch_regimes.py) instead of
    from the host reader's command tables"""

    def __init__(self, vg, ctx, font, positions, gvar_advances=True, device_stores=False):
        self.positions = [list(p) for p in positions]
        self.mgr = vg.FontManager(False)
        self.mgr.set_gvar_advances(gvar_advances)
        self.fids = [self.mgr.add_font_instance_normalized(f"P{k}", font, p) for k, p in enumerate(self.positions)]
        if device_stores and self.fids:
            self.stores, status, _ = ctx.fonts_create_gvar(self.mgr.gvar_font_desc(self.fids[0]), self.positions)
            assert all(s == 0 for s in status) and all(self.stores)
        else:
            self.stores = []
            for fid in self.fids:
                d = self.mgr.command_font_desc(fid)
                self.stores.append(ctx.font_create_commands(d["cmd_off"], d["dat_off"], d["kinds"], d["coords"]))
        self.tables = [self.mgr.family_tables_desc(fid, 0) for fid in self.fids]
        self.variation = [self.mgr.family_variation_desc(fid, 0) for fid in self.fids]
        self.gvar = [self.mgr.family_gvar_desc(fid, 0) for fid in self.fids]
        self.entries = [self.mgr.family_desc(fid) for fid in self.fids]

    @property
    def face(self):
        """the one face's cmap and hmtx: the same bytes at every position"""
        first = self.tables[0]
        for t in self.tables[1:]:
            assert bytes(t["cmap"]) == bytes(first["cmap"]) and bytes(t["hmtx"]) == bytes(first["hmtx"])
        return first

    def want(self, ctx, p, mixed=False, store=None):
        """the yardstick of position p: vgsdf_family_create over the reader's entries"""
        make = ctx.family_create_mixed if mixed else ctx.family_create
        return make([store or self.stores[p]], *[self.entries[p][k] for k in ENTRY_KEYS])

    def batched(self, ctx, mixed=False, variation="own", gvar="own", **override):
        """the batched call as the façade would state it: the records of every position, the gvar description of the first"""
        var = self.variation if variation == "own" else variation
        if var is not None and not any(var):
            var = None
        g = (self.gvar[0] if self.gvar else None) if gvar == "own" else gvar
        return ctx.families_create_tables(self.stores, self.face, var, g, self.positions if g is not None else None, mixed=mixed, **override)


def assert_same(ctx, got, want, entries):
    a, b = ctx.family_read(got), ctx.family_read(want)
    for k in ARRAYS:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    for k in ENTRY_KEYS:
        assert a[k].tobytes() == np.ascontiguousarray(entries[k]).tobytes(), k
    assert got.device_bytes == want.device_bytes and got.count(0, 0xFFFF) == len(entries["code_point"])
    assert got.count(0x20, 0x17F) == want.count(0x20, 0x17F)


def assert_every_position(ctx, placed, families, statuses, mixed=False):
    """every out[p] against its yardstick; -> the advances per position (bytes)"""
    assert statuses == [0] * len(placed.stores) and all(families)
    advances = []
    for p, got in enumerate(families):
        want = placed.want(ctx, p, mixed)
        assert_same(ctx, got, want, placed.entries[p])
        advances.append(np.ascontiguousarray(placed.entries[p]["advance"]).tobytes())
        want.free()
    return advances


def free_all(families):
    for f in families:
        if f is not None:
            f.free()


__all__ = ["G", "NI", "P", "V"]
