"""The decoder tail's routing mirror and case table (tests/head_instances.py) against the source they describe and the library's host-only
queries, which answer without a GPU: the conditions and constants the mirror copies are still spelled that way in csrc/head.hip and in
csrc/loss_kernels.hpp (the loss kernels' geometry, fold and tiling, which head.hip shares with focal.hip), the
kernels the source launches are the ones the cases reach, the workspace sizes and the fused head's predicate equal the library's over a
grid of shapes, the footprint of every admitted pair of maps fits the fused head's LDS tile and covers every image row, and every case
has the property it is there for."""
import os
import re

import numpy as np
import pytest

import head_instances as HI

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mliis_amd", "csrc", "head.hip")
LOSS_HEADER = os.path.join(os.path.dirname(SOURCE), "loss_kernels.hpp")


@pytest.fixture(scope="module")
def raw():
    from mliis_amd._lib import LIB_PATH
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from mliis_amd import ops
    return ops.lib.raw


def by_name():
    return {c.name: c for c in HI.cases()}


def test_the_source_still_routes_as_the_mirror_does():
    """The constants and conditions the mirror copies, as the source spells them."""
    head, loss = open(SOURCE).read(), open(LOSS_HEADER).read()
    # what stays in head.hip is looked up there, what the loss kernels share with focal.hip in the header: a line in the wrong file fails
    for line in ("constexpr int kResizeRowsThreads = 512;",
                 "if ((C & 3) == 0 && (ldx & 3) == 0 && (ldy & 3) == 0 && aligned16(x) && aligned16(y)) {",
                 "if ((C & 3) == 0 && (lddx & 3) == 0 && (lddy & 3) == 0 && aligned16(dx) && aligned16(dy)) {",
                 "if (C >= 16 && Wo <= 512 && Hi <= 65535 && N <= 65535) {",
                 "const size_t lds = (size_t)Wo * 8 * sizeof(float4);",
                 "if (2.f / sh + 3.f > 4.f)",
                 "const float sh = (float)(Hi - 1) / (float)(Ho - 1), sw = (float)(Wi - 1) / (float)(Wo - 1);",
                 "const bool merged = !dice && (dlogits || pred);",
                 "int nblk = (int)((per_img + 255) / 256);",
                 "if (nblk > 1024) nblk = 1024;",
                 "long long b = (q + 255) / 256;",
                 "if (b > 4096) b = 4096;",
                 "const int tx = head_tiles(Wd), nblk = head_tiles(Hd) * tx;",
                 "if (b > a || (b == a && ib < ia)) {"):
        assert line in head and line not in loss, line
    for line in ("constexpr int kHeadTile = 8, kHeadFoot = 48;",
                 "constexpr int kPartPixels = 256 * 8;",
                 "constexpr int kPartMaxBlocks = 256;",
                 "int nblk = ceil_div(HW, kPartPixels);",
                 "if (nblk > kPartMaxBlocks) nblk = kPartMaxBlocks;",
                 "return (size_t)N * nblk * 4 + 2 * (size_t)N + 8;",
                 "return (size_t)N * head_tiles(Hd) * head_tiles(Wd) * 4 + 2 * (size_t)N + 8;",
                 "for (int n0 = 0; n0 < N; n0 += 8) {",
                 "for (int b = lane; b < nblk; b += 32) {",
                 "const int v = (int)floorf((float)(i - 1) / s) - 1;",
                 "const int v = (int)ceilf((float)(i + 1) / s) + 1;",
                 "const int fh = (int)ceilf((float)(kHeadTile + 1) / sh) + 5, fw = (int)ceilf((float)(kHeadTile + 1) / sw) + 5;",
                 "return fh <= kHeadFoot && fw <= kHeadFoot;",
                 "static inline int head_tiles(int n) { return (n + kHeadTile - 1) / kHeadTile; }"):
        assert loss.count(line) == 1 and line not in head, line
    # launch and workspace query count the partial blocks with the one part_blocks(); the geometry has one definition, in the header
    assert "const int nblk = part_blocks(HW);" in head and "const int nblk = part_blocks((long long)H * W);" in loss
    assert "size_t mliis_softmax_ce_workspace_floats(int N, int H, int W) { return loss_workspace_floats(N, H, W); }" in head
    for name in ("kHeadTile =", "kHeadFoot =", "int head_lo(", "int head_hi(", "int head_tiles(", "int head_fused_supported(", "void loss_fold("):
        assert (head.count(name), loss.count(name)) == (0, 1), name
    # the resize transposes spell the candidate range as head_lo / head_hi do
    assert head.count("(int)floorf((float)(hi - 1) / sh) - 1, ho_hi = (int)ceilf((float)(hi + 1) / sh) + 1;") == 2
    assert head.count("(int)floorf((float)(wi - 1) / sw) - 1, wo_hi = (int)ceilf((float)(wi + 1) / sw) + 1;") == 2
    # the swish-mask launches spell ew_blocks' cap inline
    assert head.count("(q + 255) / 256 > 4096 ? 4096 : (q + 255) / 256") == 2
    assert (HI.EW_MAX_BLOCKS, HI.CE_PIXELS_PER_BLOCK, HI.CE_MAX_BLOCKS, HI.CE_FOLD_IMAGES, HI.CE_FOLD_LANES) == (4096, 2048, 256, 8, 32)
    assert (HI.DARC1_MAX_BLOCKS, HI.HEAD_TILE, HI.HEAD_FOOT, HI.ROWS_MIN_C, HI.ROWS_MAX_WO, HI.ROWS_THREADS) == (1024, 8, 48, 16, 512, 512)


def test_the_kernels_the_source_launches_are_the_ones_the_cases_reach():
    src = open(SOURCE).read()
    launched = re.findall(r"hipLaunchKernelGGL\(\(?(\w+(?:<\d+>)?)\)?,", src)
    assert len(launched) == 18, launched
    assert len({n.split("<")[0] for n in launched}) == 13 == len(re.findall(r"__global__ ", src))
    reached = set()
    for c in HI.cases():
        reached |= set(HI.kernels_of(c.inst))
    assert reached == set(launched)
    assert {c.inst for c in HI.cases()} == set(HI.ROUTES)
    names = [c.name for c in HI.cases()]
    assert len(names) == len(set(names))
    assert all(len(c.why) > 3 for c in HI.cases())


def test_the_librarys_host_queries_equal_the_mirror(raw):
    ce, head, ok = raw("mliis_softmax_ce_workspace_floats"), raw("mliis_head_ce_fused_workspace_floats"), raw("mliis_head_ce_fused_supported")
    for N in (0, 1, 2, 9, 17):
        for H, W in [(0, 5), (1, 1), (9, 7), (16, 12), (224, 224), (256, 256), (257, 257), (724, 724), (725, 725), (1024, 1024), (45, 46), (2048, 1), (2049, 1)]:
            assert ce(N, H, W) == HI.softmax_ce_workspace_floats(N, H, W), (N, H, W)
        for Hd, Wd in [(0, 3), (1, 1), (2, 2), (8, 8), (9, 8), (13, 7), (18, 11), (56, 56), (57, 64), (65, 1)]:
            assert head(N, Hd, Wd) == HI.head_workspace_floats(N, Hd, Wd), (N, Hd, Wd)
    for c in HI.cases_of("softmax_ce"):
        assert ce(c.p["N"], c.p["H"], c.p["W"]) == HI.softmax_ce_workspace_floats(c.p["N"], c.p["H"], c.p["W"]) > 0
    for c in HI.cases_of("head"):
        assert head(c.p["N"], c.p["Hd"], c.p["Wd"]) == HI.head_workspace_floats(c.p["N"], c.p["Hd"], c.p["Wd"]) > 0
        assert bool(ok(c.p["Hd"], c.p["Wd"], c.p["H"], c.p["W"])) == (c.inst == "head")
    # the predicate is separable: one axis against an admitted other axis
    for Hd in range(2, 65):
        for H in range(2, 301):
            want = HI.head_supported(Hd, Hd, H, H)
            assert bool(ok(Hd, Hd, H, H)) == want, (Hd, H)
            assert bool(ok(Hd, 8, H, 8)) == want == bool(ok(8, Hd, 8, H)) == HI.head_supported(8, Hd, 8, H), (Hd, H)
    assert not ok(1, 8, 8, 8) and not ok(8, 8, 1, 8) and not HI.head_supported(1, 8, 8, 8) and not HI.head_supported(8, 8, 8, 1)


def test_the_footprint_of_every_admitted_pair_fits_the_tile_and_covers_every_row():
    worst, at, admitted = 0, None, 0
    for Hd in range(2, 130):
        for H in range(2, 700):
            if not HI.head_supported(Hd, 8, H, 8):
                continue
            admitted += 1
            f = HI.head_footprint(Hd, H)
            assert f <= HI.HEAD_FOOT, (Hd, H, f)
            assert HI.head_uncovered(Hd, H) == 0, (Hd, H)
            if f > worst:
                worst, at = f, (Hd, H)
    assert admitted > 20000
    assert (worst, at) == (47, (18, 81)), (worst, at)
    assert HI.head_supported(11, 11, 48, 48) and not HI.head_supported(11, 11, 49, 49)
    assert HI.head_supported(8, 11, 8, 48) and not HI.head_supported(8, 11, 8, 49)


def test_every_resize_case_has_its_property():
    c = by_name()
    quads = lambda p, h, w, v: p["N"] * p[h] * p[w] * (p["C"] // v)      # noqa: E731
    assert [x.inst for x in HI.cases_of("resize_fwd")] == ["resize_fwd_k<4>", "resize_fwd_k<2>", "resize_fwd_k<4>", "resize_fwd_k<2>", "resize_fwd_k<4>",
                                                          "resize_fwd_k<4>"]
    lo, hi, ld = HI.SLICE
    assert (hi - lo) % 4 == 0 and ld % 4 == 0 and (lo * 4) % 8 == 0 and (lo * 4) % 16 != 0          # only the alignment sends it to <2>
    for name in ("fwd2-misaligned-slice", "bwd2-misaligned-slice"):
        p = c[name].p
        assert p["sliced"] and p["C"] == hi - lo and c[name].inst.endswith("<2>")
        assert HI.route_resize_fwd(p["C"], ld, ld, True) == "resize_fwd_k<4>"
        assert HI.route_resize_bwd(p["N"], p["Hi"], p["Wi"], p["Ho"], p["Wo"], p["C"], ld, ld, True) == "resize_bwd_k<4>"
    assert c["fwd4-hi1"].p["Hi"] == 1 and c["fwd2-mixed"].p["C"] % 4 == 2
    p = c["fwd2-mixed"].p
    assert p["Hi"] < p["Ho"] and p["Wi"] > p["Wo"]
    p = c["fwd4-identity"].p
    assert (p["Hi"], p["Wi"]) == (p["Ho"], p["Wo"])
    p = c["fwd4-grid-stride"].p
    assert quads(p, "Ho", "Wo", 4) == 1105920 > HI.EW_MAX_BLOCKS * 256 == 1048576 and HI.ew_blocks(quads(p, "Ho", "Wo", 4)) == 4096
    assert 4 * p["N"] * p["Ho"] * p["Wo"] * p["C"] < 18 << 20
    # backward
    assert [x.inst for x in HI.cases_of("resize_bwd")] == ["resize_bwd_rows_k<12>", "resize_bwd_rows_k<12>", "resize_bwd_k<4>", "resize_bwd_rows_k<4>",
                                                          "resize_bwd_rows_k<4>", "resize_bwd_k<4>", "resize_bwd_k<2>", "resize_bwd_k<2>"]
    assert (HI.BWD_PAD * 4) % 16 == 0
    p = c["rows12-rounds"].p
    lo_, hi_ = HI.candidates(1, p["Hi"], p["Ho"])
    assert hi_ - lo_ + 1 >= 60 and HI.cdiv(hi_ - lo_ + 1, 12) >= 5 and p["C"] % 32 == 4 and p["Wo"] > HI.ROWS_THREADS // 8
    p = c["rows12-lds64k"].p
    assert HI.rows_lds_bytes(p["Wo"]) == 65536 and p["Wo"] == HI.ROWS_MAX_WO
    q = c["bwd4-wo513"].p
    assert q["Wo"] == p["Wo"] + 1 and {k: v for k, v in q.items() if k != "Wo"} == {k: v for k, v in p.items() if k != "Wo"}
    for name in ("rows4-down", "rows4-mixed"):
        p = c[name].p
        assert np.float32(2) / HI.scale(p["Hi"], p["Ho"]) + np.float32(3) <= np.float32(4) and p["Hi"] > p["Ho"]
    assert c["rows4-mixed"].p["Wi"] < c["rows4-mixed"].p["Wo"] and c["rows4-mixed"].p["C"] % 32 == 20
    assert c["bwd4-narrow"].p["C"] == 12 and c["bwd2-c2"].p["C"] == 2
    # the float32 comparison is the one that decides: at 2/sh + 3 == 4 exactly (sh = 2) the batch is 4
    assert HI.route_resize_bwd(1, 9, 9, 5, 5, 16, 16, 16, True) == "resize_bwd_rows_k<4>"
    assert HI.route_resize_bwd(1, 8, 9, 5, 5, 16, 16, 16, True) == "resize_bwd_rows_k<12>"
    assert HI.route_resize_bwd(1, 9, 9, 5, 5, 12, 12, 12, True) == "resize_bwd_k<4>"
    assert HI.route_resize_bwd(1, 9, 9, 5, 5, 16, 16, 18, True) == "resize_bwd_k<2>"


def test_every_final_conv_and_swish_case_has_its_property():
    c = by_name()
    assert c["c4"].p["C"] == 4
    p = c["slice-mask"].p
    assert p["mask"] and p["ld"] > p["C"] and p["ld"] - p["off"] >= p["C"] and (p["off"] * 4) % 16 == 0 and p["ld"] % 4 == 0
    p = c["grid-stride"].p
    assert p["rows"] * (p["C"] // 4) == 1120000 > HI.EW_MAX_BLOCKS * 256 and p["ld"] > p["C"] and (p["off"] * 4) % 16 == 0
    assert 4 * p["rows"] * p["ld"] < 19 << 20
    sw = HI.cases_of("swish_mask")
    assert sorted((x.p["pre"], x.p["mask"]) for x in sw) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for x in sw:
        p = x.p
        assert p["rows"] * (p["C"] // 4) == 1080000 > HI.EW_MAX_BLOCKS * 256 and p["ld"] > p["C"] and (p["off"] * 4) % 16 == 0 and p["ld"] % 4 == 0
        assert 4 * p["rows"] * p["ld"] < 19 << 20


def test_the_wrappers_refuse_a_dense_mask_beside_a_channel_slice(raw):
    """The final conv's kernels read the mask with the leading dimension of x; the wrappers take dense masks, so beside a view with
    ld > C they must refuse before anything is launched (the slice-mask case reaches that layout through the C entry points)."""
    import torch
    from mliis_amd import ops
    p = by_name()["slice-mask"].p
    x = torch.zeros(p["rows"], p["ld"])[:, p["off"]:p["off"] + p["C"]]
    mask, dy = torch.ones(p["rows"], p["C"]), torch.zeros(p["rows"], 2)
    w, b = torch.zeros(1, 1, p["C"], 2), torch.zeros(2)
    for call in (lambda: ops.final_conv_fwd(x, w, b, mask), lambda: ops.final_conv_bwd_data(dy, w, p["C"], mask, out=x),
                 lambda: ops.final_conv_bwd_filter(x, dy, mask)):
        with pytest.raises(ops.MliisError, match="dense activation"):
            call()


def test_every_loss_case_has_its_property():
    c = by_name()
    forms = {(x.p["dice"], x.p["grad"], x.p["pred"]) for x in HI.cases_of("softmax_ce") if x.name.startswith("form-")}
    assert forms == {(0, 1, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 0, 0), (0, 0, 0)}
    for x in HI.cases_of("softmax_ce"):
        if x.name.startswith("form-"):
            assert (x.p["N"], x.p["S"], x.p["H"], x.p["W"], x.p["idx"]) == (9, 4, 9, 7, True) and x.p["N"] > HI.CE_FOLD_IMAGES
    assert HI.softmax_ce_launches(0, 0, 1) == HI.softmax_ce_launches(0, 1, 0) == ("ce_partial_k", "ce_grad_k+fin")
    assert HI.softmax_ce_launches(1, 0, 1) == ("ce_partial_k", "ce_finalize_k", "ce_grad_k")
    assert HI.softmax_ce_launches(1, 0, 0) == HI.softmax_ce_launches(0, 0, 0) == ("ce_partial_k", "ce_finalize_k")
    p = c["n17"].p
    assert p["N"] == p["S"] == 17 > 2 * HI.CE_FOLD_IMAGES and not p["idx"] and p["dice"] and (p["H"], p["W"]) == (16, 12)
    p = c["nblk33"].p
    assert HI.softmax_ce_nblk(p["H"], p["W"]) == 33 == HI.CE_FOLD_LANES + 1 and p["H"] * p["W"] > 65536
    p = c["nblk256"].p
    assert HI.softmax_ce_nblk(p["H"], p["W"]) == 256 and p["H"] * p["W"] > 256 * 2048 and HI.cdiv(p["H"] * p["W"], 2048) == 257
    assert c["extra-loss"].p["extra"] == 0.375 and c["saturated"].p["zscale"] == 30 * c["form-111"].p["zscale"] and c["ties"].p["ties"] == 0.05
    assert c["ties"].p["pred"] and c["saturated"].p["dice"]
    # fused head
    heads = HI.cases_of("head")
    assert {x.name for x in heads if x.inst == "head-refused"} == {"refused-square", "mixed-40"}
    p = c["limit"].p
    assert HI.head_footprint(p["Hd"], p["H"]) == 47 and HI.head_supported(p["Hd"], p["Wd"], p["H"], p["W"])
    assert not HI.head_supported(p["Hd"], p["Wd"], p["H"], p["W"] + 1) and (p["Hd"], p["Wd"], p["H"], p["W"]) == (18, 11, 81, 48)
    p = c["refused-square"].p
    assert (p["Hd"], p["Wd"], p["H"], p["W"]) == (11, 11, 49, 49) and HI.head_supported(11, 11, 48, 48)
    p = c["n9"].p
    assert p["N"] == 9 > HI.CE_FOLD_IMAGES and p["ls"] == 0.1 and (p["Hd"], p["Wd"], p["H"], p["W"]) == (13, 7, 37, 28)
    assert c["hd2"].p["Hd"] == 2 and not c["hd2"].p["idx"] and sum(not x.p["idx"] for x in heads) == 1
    p, q = c["mixed-40"].p, c["mixed-39"].p
    assert (p["Hd"], p["Wd"], p["H"], p["W"]) == (20, 9, 9, 40) and (q["Hd"], q["Wd"], q["H"], q["W"]) == (20, 9, 9, 39)
    assert HI.head_footprint(9, 40) <= HI.HEAD_FOOT          # (the columns would fit the tile: the predicate is the conservative side)
    assert q["Hd"] > q["H"] and q["Wd"] < q["W"] and c["mixed-39"].inst == "head"
    p = c["identity"].p
    assert (p["Hd"], p["Wd"]) == (p["H"], p["W"]) == (21, 21)
    for x in heads:
        if x.inst == "head":      # more than one tile per image but for hd2, non-square tile grids among them
            assert HI.head_tiles(x.p["Hd"]) * HI.head_tiles(x.p["Wd"]) > 1 or x.name == "hd2"
    assert any(HI.head_tiles(x.p["Hd"]) != HI.head_tiles(x.p["Wd"]) for x in heads if x.inst == "head")


def test_every_darc1_case_has_its_property():
    c = by_name()
    stride = HI.DARC1_MAX_BLOCKS * 256
    for x in HI.cases_of("darc1"):
        p = x.p
        per_img = p["H"] * p["W"] * 2
        assert all(0 <= q < per_img for q in p["plant"]) and list(p["plant"]) == sorted(set(p["plant"])), x.name
    assert HI.darc1_nblk(30) == 1 and c["one-block"].p["H"] * c["one-block"].p["W"] * 2 == 30
    p = c["last-block"].p
    assert HI.darc1_nblk(960) == 4 and p["plant"][0] // 256 == 3 and p["N"] == 8
    assert HI.BIG == 263538 > stride == 262144 and HI.darc1_nblk(HI.BIG) == 1024 and HI.cdiv(HI.BIG, 256) == 1030
    for name in ("stride-second", "stride-first", "tie-thread", "tie-apply-thread"):
        assert c[name].p["H"] * c[name].p["W"] * 2 == HI.BIG and c[name].p["N"] == 2
    assert c["stride-second"].p["plant"][0] >= stride > c["stride-first"].p["plant"][0]
    a, b = c["tie-thread"].p["plant"]
    assert b - a == stride                                             # the same thread, its first and its second pass
    a, b = c["tie-lanes"].p["plant"]
    assert a // 256 == b // 256 and a % 64 != b % 64                   # one block, two lanes
    a, b = c["tie-blocks"].p["plant"]
    assert a // 256 != b // 256 and b < stride and HI.darc1_nblk(960) <= 256          # two blocks, each with a thread of its own in the apply kernel
    a, b = c["tie-apply-thread"].p["plant"]
    assert b < stride and (b // 256 - a // 256) == 256                 # blocks b0 and b0 + 256: one thread of darc1_apply_k folds both
    assert c["zero-sign"].p["zero"] and c["zero-sign"].p["N"] > 2
    assert {x.p["outs"] for x in HI.cases_of("darc1")} == {"both", "dlogits", "out"}
