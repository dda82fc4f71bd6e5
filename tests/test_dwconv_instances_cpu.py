"""The plain-depthwise instance table and routing mirror (tests/dwconv_instances.py) against the source they describe and the library's
workspace query, which is host code and answers without a GPU: the table is what the launch sites of csrc/dwconv.hip can name, every
instance is reached by a case or carries the reason why no call below 2 GiB launches it, the mirror's filter-gradient geometry counts
the library's slabs, and every case has the property it is there for -- tails and tile counts, pt != pl, a buffer size that tells two
routes apart, idle lanes, a partial channel group, a walk of two strips with a partial last block."""
import itertools
import os
import re

import pytest

import dwconv_instances as DI

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mliis_amd", "csrc", "dwconv.hip")
BASELINE = [(8, H, H, C, k, s) for k, s, H, C in [(3, 1, 112, 32), (3, 2, 112, 96), (3, 1, 56, 144), (5, 2, 56, 144), (5, 1, 28, 240), (3, 2, 28, 240),
                                                  (3, 1, 14, 480), (5, 1, 14, 480), (5, 1, 14, 672)]]      # test_dwconv_baseline_shapes
ODD = [(1, 1, 1, 4), (2, 41, 63, 44), (1, 33, 61, 36), (3, 7, 9, 260), (5, 19, 23, 1028), (64, 112, 112, 32), (2, 225, 225, 96), (1, 3, 1025, 8)]


@pytest.fixture(scope="module")
def workspace_floats():
    from mliis_amd._lib import LIB_PATH
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from mliis_amd import ops
    return ops.lib.raw("mliis_dwconv_bwd_filter_workspace_floats")


def cases_of(inst):
    return [c for c in DI.cases() if c.inst == inst]


def test_the_table_is_what_the_launch_sites_can_name():
    src = open(SOURCE).read()
    launches = re.findall(r"hipLaunchKernelGGL\(\((\w+)<([^>]*)>\)", src)
    tile_lines = [a for n, a in launches if n == "dwconv_tile_k"]
    assert tile_lines == ["3, 1, 7, 16, 4, FLIP, STATS, DIL, BNB", "5, 1, 7, 16, 4, FLIP, STATS, DIL, BNB", "5, 2, 7, 7, 1, FLIP, STATS, false, false"]
    assert sorted(a for n, a in launches if n == "KERNEL") == ["3, 1, kTW", "3, 2, kTW", "5, 1, kTW", "5, 2, kTW"]
    assert len(launches) == 7, launches
    dispatched = [n for n in re.findall(r"DW_DISPATCH\((\w+),", src) if n != "KERNEL"]
    assert sorted(dispatched) == ["dwconv_bwd_data_k", "dwconv_bwd_filter_k", "dwconv_fwd_k", "dwconv_fwd_stats_k"]
    forms = re.findall(r"launch_dw_tile<([^>]*)>\(", src)
    assert forms == ["false, true", "false, false", "true, false, false, true", "true, false, true, true", "true, false, false", "true, false, true"]
    assert "template <bool FLIP, bool STATS, bool DIL = false, bool BNB = false>\nstatic void launch_dw_tile(" in src
    # the names the source can spell, by substitution, are the table's
    named = {"{}<{}>".format(n, a.replace("kTW", str(DI.TW))) for n in dispatched for a in ("3, 1, kTW", "3, 2, kTW", "5, 1, kTW", "5, 2, kTW")}
    for form in forms:
        flags = (form.split(", ") + ["false", "false"])[:4]
        for line in tile_lines:
            for name, value in zip(("FLIP", "STATS", "DIL", "BNB"), flags):
                line = line.replace(name, value)
            named.add("dwconv_tile_k<{}>".format(line))
    assert named == {DI.kernel_name(i) for i in DI.INSTANCES}
    assert len(DI.INSTANCES) == len(set(DI.INSTANCES)) == len(named) == 31
    assert [sum(i.kernel == kern for i in DI.INSTANCES) for kern in ("fwd", "fwd_stats", "bwd_data", "bwd_filter", "tile")] == [4, 4, 4, 4, 15]
    assert tuple(tuple(f == "true" for f in (form.split(", ") + ["false", "false"])[:4]) for form in forms) == DI.TILE_FORMS


def test_the_source_still_routes_as_the_mirror_does():
    """The constants and conditions the mirror copies, as the source spells them."""
    src = open(SOURCE).read()
    for line in ("constexpr int kTW = 4;", "d.toh = 7;", "d.tow = stride == 1 ? 16 : 7;", "long long want = 512 / g.ny;",
                 "const int nblk = (int)((strips + 31) / 32);", "g.QB = Q < 64 ? Q : 64;", "g.RP = 256 / g.QB;",
                 "const bool tiled = k == 5 && stride == 1 && (long long)N * H * W * C * 4 < (1LL << 31) && tile.blocks < (1LL << 31);",
                 "if (tiled && (size_t)tile.blocks * 2 * C <= stats_floats) {",
                 "const DwTile tile = dw_tile(N, H, W, 1);",
                 "const bool small = (long long)N * H * W * C * 4 < (1LL << 31) && tile.blocks < (1LL << 31);",
                 "&& (size_t)tile.blocks * 2 * C <= part_floats;",
                 "if (small && (k == 5 || fuse)) {", "if (nblk) *nblk = 0;"):
        assert line in src, line
    assert (DI.TW, DI.TOH, DI.TOW, DI.TS, DI.STATS_STRIPS, DI.FILTER_WANT, DI.LIMIT) == (4, 7, 16, 4, 32, 512, 1 << 31)
    # every backward-data launch hands launch_dw_tile the stride-1 geometry, the forward launches the layer's stride
    assert re.findall(r"launch_dw_tile<true[^>]*>\(tile, (\w+), C,", src) == ["1"] * 4
    assert re.findall(r"launch_dw_tile<false[^>]*>\(tile, (\w+), C,", src) == ["stride"] * 2
    assert DI.same_pad(16, 33, 3, 2) == (8, 17, 0, 1) and DI.same_pad(16, 33, 5, 2) == (8, 17, 1, 2) and DI.same_pad(1, 1, 5, 2) == (1, 1, 2, 2)


def test_every_declared_instance_is_reached_or_has_a_reason():
    cases = DI.cases()
    reached = {DI.launched(c)[0] for c in cases}
    assert not (reached & set(DI.UNREACHABLE))
    assert reached | set(DI.UNREACHABLE) == set(DI.INSTANCES)
    assert len(reached) == 21 and len(DI.UNREACHABLE) == 10
    assert all(len(why) > 40 and why.endswith(".") and " " in why for why in DI.UNREACHABLE.values())
    ids = [DI.case_id(c) for c in cases]
    assert len(ids) == len(set(ids))
    for c in cases:
        inst, nblk = DI.launched(c)
        if c.kind != "fallback":
            assert inst == c.inst, DI.case_id(c)
        assert (c.k, c.s) == DI.layer_of(c.inst)
        assert 4 * c.shape[0] * c.shape[1] * c.shape[2] * c.shape[3] <= 21 << 20      # tiny tensors: at most 20 MiB, most a few KiB
    # what the mirror says about the unreachable ones: no buffer size and no shape below 2 GiB routes there
    for N, H, W, C in [DI.RAGGED, DI.EVEN, DI.MIXED, DI.GROUPS, (8, 112, 112, 96)] + list(DI.TINY):
        for (k, s), floats in itertools.product(DI.KS, (None, 1 << 24)):
            assert DI.fwd_route(N, H, W, C, k, s, floats)[0] not in DI.UNREACHABLE
            for with_bn in (False, True):
                assert DI.bwd_data_route(N, H, W, C, k, s, with_bn, floats or 0)[0] not in DI.UNREACHABLE
    # ... and a tensor of 2 GiB does reach the sliding-window 5x5 kernels
    assert DI.fwd_route(64, 512, 512, 32, 5, 1, None)[0] == DI.sliding("fwd", 5, 1)
    assert DI.bwd_data_route(64, 512, 512, 32, 5, 2, False, 0)[0] == DI.sliding("bwd_data", 5, 2)


def test_every_reached_instance_has_the_kinds_it_needs():
    for i in DI.INSTANCES:
        if i in DI.UNREACHABLE:
            continue
        mine = cases_of(i)
        kinds = {c.kind for c in mine}
        k, s = DI.layer_of(i)
        if i.kernel == "bwd_filter":
            assert kinds == {"idle", "groups", "walk"}, (i, kinds)
            assert {c.shape[3] for c in mine if c.kind == "idle"} == {40, 12}
            continue
        want = {"ragged", "tiny"} | ({"even", "mixed"} if s == 2 else set()) | ({"fallback"} if i.bnb else set())
        assert kinds == want, (i, kinds)
        tiny = {c.shape for c in mine if c.kind == "tiny"}
        assert tiny == ({DI.TINY_GAP, DI.TINY[1]} if i == DI.sliding("fwd_stats", 5, 1) else set(DI.TINY)), (i, tiny)
        assert {c.shape for c in mine if c.kind == "ragged"} == {(2, 15, 33, 40)}
        assert all((c.floats is not None) == (i.kernel == "fwd_stats" or i.stats or i.bnb) for c in mine)
        if s == 2:
            assert {c.shape for c in mine if c.kind == "even"} == {(2, 16, 34, 40)} and {c.shape for c in mine if c.kind == "mixed"} == {(2, 16, 33, 40)}
        if i.bnb:
            assert {c.shape for c in mine if c.kind == "fallback"} == ({DI.RAGGED, DI.MIXED} if i.dil else {DI.RAGGED})


def test_the_mirror_counts_the_librarys_filter_gradient_slabs(workspace_floats):
    shapes = {c.shape for c in DI.cases()} | set(ODD)
    for (N, H, W, C), (k, s) in itertools.product(sorted(shapes), DI.KS):
        assert DI.filter_geom(N, H, W, C, k, s).nblk * k * k * C == workspace_floats(N, H, W, C, k, s) > 0, (N, H, W, C, k, s)
    for N, H, W, C, k, s in BASELINE:
        assert DI.filter_geom(N, H, W, C, k, s).nblk * k * k * C == workspace_floats(N, H, W, C, k, s) > 0, (N, H, W, C, k, s)
    for c in DI.cases():
        if c.inst.kernel == "bwd_filter":
            assert c.floats == workspace_floats(*c.shape, c.k, c.s), DI.case_id(c)


def test_ragged_tiny_and_stride_2_cases_have_their_tails():
    for c in DI.cases():
        N, H, W, C = c.shape
        Ho, Wo, pt, pl = DI.same_pad(H, W, c.k, c.s)
        e = DI.entry_of(c)
        if e == "bwd_filter":
            continue
        th, tw = (Ho, Wo) if e == "fwd" else (H, W)          # what the tiles (and the strips of the sliding-window kernels) cover
        if c.shape == DI.RAGGED:
            t = DI.tile_geom(N, th, tw)
            assert N > 1 and C % 32 == 8 and DI.cdiv(C, 32) == 2
            assert th % DI.TOH and tw % DI.TOW and tw % DI.TS, DI.case_id(c)
            if (th, tw) == (15, 33):
                assert (t.tiles_y, t.tiles_x, t.blocks) == (3, 3, 18) and DI.strips_of(N, th, tw) == 270
            else:
                assert (th, tw, t.tiles_y, t.tiles_x) == (8, 17, 2, 2)
        if c.kind == "tiny":
            assert H <= c.k and W <= c.k and H * W < c.k * c.k and C in (4, 12)      # no output whose window lies inside the map
        if c.kind == "even":
            assert c.s == 2 and H % 2 == 0 and W % 2 == 0 and pt == pl == (c.k - 2) // 2
        if c.kind == "mixed":
            assert c.s == 2 and pt != pl and (pt, pl) == {3: (0, 1), 5: (1, 2)}[c.k]


def test_a_buffer_size_tells_the_two_statistics_layouts_apart():
    for c in DI.cases():
        N, H, W, C = c.shape
        e = DI.entry_of(c)
        inst, nblk = DI.launched(c)
        if e == "fwd" and c.floats is not None:
            Ho, Wo, _, _ = DI.same_pad(H, W, c.k, c.s)
            sliding, tiles = DI.stats_blocks(N, H, W, c.k, c.s), DI.tile_geom(N, Ho, Wo).blocks
            if c.inst == DI.sliding("fwd_stats", 5, 1):
                # reached only in the gap: room for its own layout, one float short of the tile layout
                assert nblk == sliding < tiles and sliding * 2 * C <= c.floats == tiles * 2 * C - 1, DI.case_id(c)
                assert DI.fwd_route(N, H, W, C, 5, 1, c.floats + 1) == (DI.tile(5, 1, False, True), tiles)
                if c.shape == DI.RAGGED:
                    assert (sliding, tiles, c.floats) == (9, 18, 1439) and 270 - 8 * 32 == 14          # live lanes of the last block
            elif c.inst.stats:
                assert nblk == tiles and c.floats == tiles * 2 * C
                assert tiles == sliding or DI.fwd_route(N, H, W, C, 5, 1, c.floats - 1)[0] == DI.sliding("fwd_stats", 5, 1)
                if c.shape == DI.RAGGED:
                    assert tiles != sliding
            else:
                assert nblk == sliding and c.floats == sliding * 2 * C
                with pytest.raises(ValueError):
                    DI.fwd_route(N, H, W, C, c.k, c.s, c.floats - 1)
                if c.shape == DI.RAGGED:
                    assert nblk % 8 != 0 and DI.strips_of(N, Ho, Wo) % 32 != 0     # xcd_remap off a multiple of 8, a partly idle last block
        if e == "bwd_data_bn":
            tiles = DI.tile_geom(N, H, W).blocks
            if c.kind == "fallback":
                assert nblk == 0 and c.floats == tiles * 2 * C - 1 and tiles > 1
                assert inst == (DI.sliding("bwd_data", c.k, c.s) if c.k == 3 else DI.tile(5, 1, True, False, c.s == 2, False)), DI.case_id(c)
            else:
                assert inst == c.inst and nblk == tiles and c.floats == tiles * 2 * C
        if e == "bwd_data":
            assert nblk == 0 and c.floats is None


def test_filter_gradient_cases_have_idle_lanes_partial_groups_and_walks():
    for c in DI.cases():
        if c.inst.kernel != "bwd_filter":
            continue
        g = DI.filter_geom(*c.shape, c.k, c.s)
        assert g.QB * g.RP + g.idle_lanes == 256 and g.items_per_block % g.RP == 0 and 1 <= g.last_block_items <= g.items_per_block
        if c.kind == "idle":
            assert g.idle_lanes > 0 and g.ny == 1 and g.max_walk == 1, (DI.case_id(c), g)
            assert (g.QB, g.RP, g.idle_lanes) == {40: (10, 25, 6), 12: (3, 85, 1)}[c.shape[3]]
        if c.kind == "groups":
            assert (g.QB, g.RP, g.ny, g.last_group_quads) == (64, 4, 2, 8), (DI.case_id(c), g)
            if c.shape == DI.GROUPS and c.s == 1:
                assert (g.items, g.items_per_block, g.nblk, g.last_block_items) == (270, 4, 68, 2)
        if c.kind == "walk":
            assert g.max_walk >= 2 and g.last_block_items < g.items_per_block and g.ny == 2 and g.last_group_quads == 8, (DI.case_id(c), g)
            assert (g.items, g.items_per_block, g.nblk, g.last_block_items, g.nblk % 8) == (1122, 8, 141, 2, 5)
    # every filter instance sees a partial last block among its groups cases
    for k, s in DI.KS:
        mine = [c for c in cases_of(DI.sliding("bwd_filter", k, s)) if c.kind == "groups"]
        assert any(DI.filter_geom(*c.shape, k, s).last_block_items < DI.filter_geom(*c.shape, k, s).items_per_block for c in mine), (k, s)
    # the thresholds themselves: one strip per thread until N * Ho * ceil(Wo / 4) > (512 / ny) * RP
    assert DI.filter_geom(1, 1, 4 * 512 * 4, 256, 3, 1).max_walk == 1 and DI.filter_geom(1, 1, 4 * 512 * 4 + 1, 256, 3, 1).max_walk == 2
