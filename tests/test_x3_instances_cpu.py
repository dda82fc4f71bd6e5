"""The split-product instance manifest (tests/x3_instances.py) against the launch switches of csrc/conv_x3.hip and against the
library's planner: the declared lists are the switches' cases, the Python mirror of x3_pick_nt / x3_plan equals the library on every
searched shape and on a grid of further ones, every declared instance is reached, the searched shapes have the tails their kind
promises, the stream-K cuts the GPU file launches cover every class of cut, and the contract refusals come back from the host path.
The planner queries answer without a GPU (the CU count falls back to the MI355X's 256)."""
import ctypes as C
import os

import pytest

import x3_instances as X


@pytest.fixture(scope="module")
def lib():
    from mliis_amd._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return lib


@pytest.fixture(scope="module")
def filters(lib):
    return X.search_filter()


# ------------------------------------------------------------------------------------------------ manifest
def test_manifest_equals_the_launch_switches():
    conv_nt, kernels, filt_nt, widths = X.parse_switches()
    assert conv_nt == X.X3_NT and filt_nt == X.FILTER_NT
    assert kernels == ("conv_x3_k", "x3_fixup_k")                      # one case launches the pair
    assert tuple(str(w) for w in widths) == X.FILTER_BODIES[:2]
    assert len(X.declared()) == 9 + 9 + 9 + 15                          # conv_x3_k in two directions, the fix-up, the filter bodies
    assert set(X.UNREACHABLE) <= X.declared()
    assert all("plan" in why and len(why) > 40 for why in X.UNREACHABLE.values())


def test_the_parser_sees_an_added_case(tmp_path):
    """A case added to either switch (or a third body width) without a manifest entry must fail the comparison above."""
    src = open(X.SOURCE).read()
    edited = src.replace("    default: L(9)\n", "    case 9: L(9)\n    default: L(10)\n", 1)
    edited = edited.replace("    case 8: L(8)\n    default: return false;", "    case 8: L(8)\n    case 9: L(9)\n    default: return false;", 1)
    edited = edited.replace("else conv_filter_x3_body<NT, 128>(p, sm,", "else if (p.C > 999) conv_filter_x3_body<NT, 512>(p, sm, bx, 0, 0);\n  else conv_filter_x3_body<NT, 128>(p, sm,", 1)
    assert edited.count("L(10)") == 1 and edited.count("case 9: L(9)") == 2 and edited.count("<NT, 512>") == 1
    p = tmp_path / "conv_x3.hip"
    p.write_text(edited)
    conv_nt, _, filt_nt, widths = X.parse_switches(str(p))
    assert conv_nt == X.X3_NT + (10,) and filt_nt == X.FILTER_NT + (9,) and widths == (128, 256, 512)


# ------------------------------------------------------------------------------------------------ mirror == library
def _agrees(s):
    p, lp = X.plan_of(s), X.lib_plan(s)
    assert (lp[0], lp[1], lp[2], lp[7], lp[4], lp[5], lp[6]) == tuple(p) and lp[3] == 0, (s, p, lp)
    assert X.lib_workspace_floats(s) == X.workspace_floats(p), (s, p)
    return p


def _cuts_are_consistent(p, s):
    """conv_x3_k and x3_fixup_k compute a tile's slots independently: every slot the fix-up folds is written exactly once, none
    beyond smax, and the segments tile the K range of every tile without gap or overlap."""
    nsl, w = X.slots(p), X.written_slots(p)
    assert all(sorted(w[rt]) == list(range(nsl[rt])) and nsl[rt] <= p.smax for rt in range(p.gx * p.gy)), (s, p)
    cover = {}
    for part, rt, c0, c1 in X.segments(p):
        assert 0 <= c0 < c1 <= p.nchunks and cover.get(rt, 0) == c0, (s, p, part, rt, c0, c1)
        cover[rt] = c1
    assert all(cover[rt] == p.nchunks for rt in range(p.gx * p.gy)), (s, p)


def test_mirror_equals_the_library_on_every_searched_shape_and_on_a_grid(lib):
    from mliis_amd import ops
    for s in X.all_conv_shapes():
        p = _agrees(s)
        _cuts_are_consistent(p, s)
        assert ops.conv2d_x3_kernel_name(s.N, s.H, s.W, s.Cred, s.Nout, s.ksize) == "conv_x3_k<%d>" % p.nt
    n, seen = 0, set()
    for N, H, W in ((1, 1, 1), (1, 3, 5), (2, 7, 9), (1, 16, 16), (1, 7, 37), (3, 14, 14), (8, 14, 14), (2, 28, 28), (8, 56, 56), (16, 96, 96)):
        for nout in list(range(4, 300, 12)) + [16, 32, 48, 112, 136, 144, 224, 288]:
            for k in (1, 3):
                for cred in (32, 36, 40, 64, 100, 112, 136, 224, 360, 672, 1252, 3644, 7284):
                    s = X.Shape(N, H, W, cred, nout, k, 1)
                    p = _agrees(s)
                    if p.parts * p.gx * p.gy <= 1 << 16:
                        _cuts_are_consistent(p, s)
                    seen.add(p.nt)
                    n += 1
    assert n >= 3000 and seen == set(X.X3_NT)


def test_three_plans_by_hand_from_the_library(lib):
    """3x3 on a 37-pixel map, worked by hand from x3_plan: (Cred 3644, Nout 260): 1025 chunks x 2 column tiles >= 2048, NT stays 9;
    (1820, 196): 512 chunks, NT 7 -> 4 with four column tiles; (2428, 292): 683 chunks x 3 column tiles, NT stays 7 -- asked of the
    library, not of the mirror."""
    for cred, nout, nt in ((3644, 260, 9), (1820, 196, 4), (2428, 292, 7)):
        assert X.lib_plan(X.Shape(1, 1, 37, cred, nout, 3, 1))[0] == nt


# ------------------------------------------------------------------------------------------------ reached | unreachable == declared
def test_every_declared_instance_is_reached_or_has_a_reason(filters):
    hit = set(X.reached_conv()) | set(filters)
    declared, never = X.declared(), set(X.UNREACHABLE)
    assert hit <= declared, sorted(hit - declared)
    assert not (hit & never), sorted(hit & never)
    assert hit | never == declared, sorted(declared - hit - never)
    assert set(X.searched()) == {(nt, d, kind) for nt in X.X3_NT for d in X.DIRECTIONS for kind in X.KINDS}


def test_searched_shapes_have_their_tails_and_stay_small():
    for (nt, direction, kind), s in X.searched().items():
        p = X.plan_of(s)
        assert p.nt == nt and X.cost(s) <= X.MAX_COST, (nt, direction, kind, s)
        assert s.Cred >= 32 and s.Cred % 4 == 0 and s.Nout % 4 == 0
        if kind == "edge":
            assert set(X.edge_missing(s, p)) == X.EDGE_SHORTFALL.get(nt, set()), (nt, direction, s, X.edge_missing(s, p))
            assert s.dil == 1 + nt % 2
        else:
            assert set(X.loop_missing(s, p, direction)) == X.loop_shortfall(nt, direction), (nt, direction, s, X.loop_missing(s, p, direction))
    # the narrower last column tile at the column counts the kernel's b_lim path was written for
    for nt, lo, hi in ((6, 164, 176), (7, 196, 208), (8, 228, 240), (9, 260, 272)):
        for direction in X.DIRECTIONS:
            s = X.searched()[(nt, direction, "edge")]
            assert lo <= s.Nout <= hi or ((s.Nout + 15) // 16) % nt != 0, (nt, s)
    # the two kinds of one instance differ, and one direction of the loop kind has whole row tiles wherever the cap lets it
    assert all(X.searched()[(nt, d, "edge")] != X.searched()[(nt, d, "loop")] for nt in X.X3_NT for d in X.DIRECTIONS)
    assert all(X.rows(X.searched()[(nt, "fwd", "loop")]) % X.BM == 0 for nt in (1, 2, 3))
    # test_exact_b_terms relies on it: the edge kind is the 3x3 one, the loop kind the 1x1 one
    assert all(s.ksize == (3 if kind == "edge" else 1) for (_, _, kind), s in X.searched().items())
    # rows of the loop shapes: at least one full 256-row tile up to NT = 5, 65 rows from NT = 6 on; FULL_TILE_CASES give 6 and 8 a full tile
    assert all((X.rows(s) >= X.BM) == (nt <= 5) for (nt, _, kind), s in X.searched().items() if kind == "loop")
    assert sorted(X.plan_of(s).nt for s in X.FULL_TILE_CASES) == [6, 8]
    assert all(X.rows(s) == X.BM and s.ksize == 3 and X.MAX_COST < X.cost(s) <= X.FULL_TILE_COST for s in X.FULL_TILE_CASES)


def test_every_cut_class_is_produced_by_a_gpu_case():
    table = X.cut_table()
    produced = set().union(*table.values())
    assert produced == set(X.CUT_CLASSES), sorted(set(X.CUT_CLASSES) - produced)
    cheap = set().union(*(table[s] for s in X.CUT_CASES))
    assert cheap == set(X.CUT_CLASSES), sorted(set(X.CUT_CLASSES) - cheap)       # the cut cases alone carry them all
    assert all(X.plan_of(s).nt <= 2 and X.cost(s) < 10 ** 7 for s in X.CUT_CASES)
    # what the comments of CUT_CASES say of single cases
    by = {s: table[s] for s in X.CUT_CASES}
    assert X.plan_of(X.CUT_CASES[0]) == X.Plan(1, 1, 1, 2, 1, 2, 2)                                   # (a): one part, two chunks
    assert any(X.plan_of(s).nchunks <= 2 and X.plan_of(s).ipp == 4 and "b" in c for s, c in by.items())   # (b) with nchunks <= 2 and ipp = 4
    assert any(s.Cred == 32 and s.ksize == 3 for s in X.CUT_CASES)
    assert any(s.H == 1 for s in X.CUT_CASES) and any(s.W == 1 for s in X.CUT_CASES)
    # a wave with no valid row: a last row tile with fewer than 225 rows; and rows of several images in one tile
    assert any(0 < X.rows(s) % X.BM <= 224 for s in X.CUT_CASES) and any(s.N > 1 and s.H * s.W < X.BM for s in X.CUT_CASES)


# ------------------------------------------------------------------------------------------------ filter gradients
def test_filter_shapes_launch_the_instance_they_are_listed_for(filters):
    assert set(filters) == {X.filter_name(nt, b) for nt in X.FILTER_NT for b in X.FILTER_BODIES}
    for name, shapes in filters.items():
        for s in shapes:
            assert X.filter_instance(s) == name and X.fcost(s) <= X.FILTER_MAX_COST, (name, s)
            tmf, nt, mt = X.filter_plan(s)[:3]
            assert tmf == 2 and (mt == 1) == name.endswith("multitap") and (s.Cin in (8, 12)) == (mt == 1)
    every = [s for shapes in filters.values() for s in shapes]
    for nt in X.FILTER_NT:   # both channel counts of the multitap form, for every column-tile count
        assert {s.Cin for s in filters[X.filter_name(nt, "multitap")]} == {8, 12}, nt
    assert any((s.N * s.H * s.W) % 32 != 0 for s in every) and any(s.N * s.H * s.W < 32 for s in every)
    assert any(52 <= s.Cout <= 64 for s in filters[X.filter_name(4, "128")]) and any(84 <= s.Cout <= 96 for s in filters[X.filter_name(6, "128")])


def test_channel_counts_that_never_take_the_split_product_filter_kernels(lib):
    """plan_filter keeps 128-channel tiles (TMF = 2, the only groups mliis_conv2d_bwd_filter_batched hands to
    conv_filter_x3_batched_k) for Cin = 128 and for a last 128-channel tile that is more than half full.  36, 100, 132 and 260 input
    channels take 64-channel tiles on every map and run the native instruction under "fp32x3" too."""
    for cin in (36, 100, 132, 260):
        for m in ((1, 5, 5), (4, 30, 30), (8, 56, 56)):
            for cout in (52, 96, 112):
                for k in (1, 3):
                    assert X.filter_instance(X.FShape(*m, cin, cout, k, 1, True)) is None
    assert X.filter_instance(X.FShape(8, 56, 56, 224, 112, 3, 1, True)) == X.filter_name(7, "256")   # the decoder's fuse conv
    assert X.filter_instance(X.FShape(8, 56, 56, 128, 112, 3, 2, True)) == X.filter_name(7, "128")
    # the 8-channel sliver of the decoder's concat at its real size plans (TMF 2, NT 2, multitap): 98 slabs x 1 column block do not fill
    # the chip, plan_filter narrows to two column tiles and the launch switch has no such case -- the native instruction.  The
    # multitap body of conv_filter_x3_batched_k runs once column blocks x slabs fill the chip (8281 pixels x 920 columns, 66049 x 68).
    assert X.filter_plan(X.FShape(8, 56, 56, 8, 112, 3, 2, True))[:3] == (2, 2, 1)
    assert X.filter_instance(X.FShape(8, 56, 56, 8, 112, 3, 2, True)) is None


# ------------------------------------------------------------------------------------------------ contract refusals (host path, no launch)
FAKE = 0x10000   # an aligned address nobody dereferences: every call below is refused before the launch


def _fwd(lib, N, H, W, cin, cout, k, image_bytes, ws_floats, dil=1):
    from mliis_amd._lib import MliisError
    nblk = C.c_int(0)
    with pytest.raises(MliisError) as e:
        lib.call("mliis_conv2d_fwd_x3", FAKE, cin, FAKE, image_bytes, None, None, FAKE, cout, N, H, W, cin, cout, k, dil, 0, None, 0, C.byref(nblk),
                 FAKE, ws_floats, None)
    return str(e.value)


def _bwd(lib, N, H, W, cin_out, cout, k, image_bytes, ws_floats):
    from mliis_amd._lib import MliisError
    with pytest.raises(MliisError) as e:
        lib.call("mliis_conv2d_bwd_data_x3", FAKE, cout, FAKE, image_bytes, FAKE, cin_out, N, H, W, cin_out, cout, k, 1, 0, FAKE, ws_floats, None)
    return str(e.value)


def test_contract_refusals_come_from_the_host_path(lib):
    """Each violation is refused by its own check (the message says which); the workspace of every call but the last pair is empty
    as well, so that nothing could be launched even if a check were lost.  The last pair -- a workspace one float short -- has nothing
    behind it: it relies on the workspace check alone, on the smallest shape there is (15 rows, one part)."""
    img = lambda cred, nout, k: lib.size("mliis_x3_image_bytes", cred, nout, k)
    assert "must be >= 32" in _fwd(lib, 1, 3, 5, 28, 16, 3, img(28, 16, 3), 0)
    assert "must be >= 32" in _bwd(lib, 1, 3, 5, 16, 28, 3, img(28, 16, 3), 0)
    assert "multiples of 4" in _fwd(lib, 1, 3, 5, 38, 16, 3, img(38, 16, 3), 0)
    assert "multiples of 4" in _fwd(lib, 1, 3, 5, 36, 18, 3, img(36, 18, 3), 0)
    assert "multiples of 4" in _bwd(lib, 1, 3, 5, 18, 36, 3, img(36, 18, 3), 0)
    assert "kernel size 5 unsupported" in _fwd(lib, 1, 3, 5, 36, 16, 5, img(36, 16, 3), 0)
    assert "dilation" in _fwd(lib, 1, 3, 5, 36, 16, 3, img(36, 16, 3), 0, dil=0)
    # an image packed for another channel window, another column count, or the other direction of a non-square weight
    assert "packed for another window" in _fwd(lib, 1, 3, 5, 36, 16, 3, img(68, 16, 3), 0)
    assert "packed for another window" in _fwd(lib, 1, 3, 5, 36, 40, 3, img(36, 16, 3), 0)
    assert img(36, 100, 3) != img(100, 36, 3)
    assert "packed for another window" in _bwd(lib, 1, 3, 5, 100, 36, 3, img(100, 36, 3), 0)
    # a workspace one float short
    s = X.Shape(1, 3, 5, 36, 16, 3, 1)
    need = X.lib_workspace_floats(s)
    assert need == X.workspace_floats(X.plan_of(s)) > 0
    assert "workspace too small" in _fwd(lib, 1, 3, 5, 36, 16, 3, img(36, 16, 3), need - 1)
    assert "workspace too small" in _bwd(lib, 1, 3, 5, 16, 36, 3, img(36, 16, 3), need - 1)


# ------------------------------------------------------------------------------------------------ the references
def test_the_float64_references_agree_with_the_oracle_ops():
    """x3_instances.conv_ref / bwd_data_ref / filter_grad_ref (im2col + matmul) against oracle.efficientlab_ref.conv2d_same and its
    autograd, 1x1 and 3x3, dilation beyond the map included."""
    import torch
    from oracle import efficientlab_ref as R
    g = torch.Generator().manual_seed(1)
    for N, H, W, cin, cout, k, dil in ((2, 5, 7, 8, 12, 3, 1), (1, 6, 4, 4, 8, 3, 2), (2, 3, 2, 8, 4, 3, 3), (3, 4, 5, 12, 8, 1, 1), (1, 1, 9, 4, 4, 3, 1)):
        x = torch.randn(N, H, W, cin, generator=g, dtype=torch.float64).requires_grad_(True)
        w = torch.randn(k, k, cin, cout, generator=g, dtype=torch.float64).requires_grad_(True)
        dy = torch.randn(N, H, W, cout, generator=g, dtype=torch.float64)
        y = R.conv2d_same(x.permute(0, 3, 1, 2), w, 1, dil).permute(0, 2, 3, 1)
        gx, gw = torch.autograd.grad(y, [x, w], dy)
        assert (X.conv_ref(x.detach(), w.detach(), dil) - y.detach()).abs().max() < 1e-12
        assert (X.bwd_data_ref(dy, w.detach(), dil) - gx).abs().max() < 1e-12
        assert (X.filter_grad_ref(x.detach(), dy, k, dil) - gw).abs().max() < 1e-12
