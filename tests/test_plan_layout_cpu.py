"""The integer launch tables of an inner step, checked where a wrong word costs nothing: plan.py's layout functions (fold regions and
rows, squeeze-excite tiles, scratch sizes) and ops.FilterBatch's tables are pure functions of (arch, N, flags) over the library's size
and eligibility queries, which are host code and answer without a GPU.  On the device a wrong word in any of them is an out-of-bounds
write."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

CASES = {"b0-224-n8": (dict(name="efficientnet-b0", size=224), 8), "b0-224-n5": (dict(name="efficientnet-b0", size=224), 5),
         "b3-224-n8": (dict(name="efficientnet-b3", size=224), 8), "b0-64-skipdec": (dict(name="efficientnet-b0", size=64, skipdec=True), 8),
         "b0-64-aspp": (dict(name="efficientnet-b0", size=64, aspp=True), 8)}


@pytest.fixture(scope="module", autouse=True)
def library():
    from mliis_amd._lib import LIB_PATH
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()


@functools.lru_cache(maxsize=None)
def layout(case):
    from mliis_amd import plan, spec
    from mliis_amd.arena import Arena
    kw, N = CASES[case]
    arch = spec.derive(kw["name"], kw["size"], [2, 4], 0.0, kw.get("aspp", False), skip_decoding=kw.get("skipdec", False))
    arena = Arena(arch, "cpu")   # (the arena's offsets are the table's `out` column)
    names = plan.layer_names(arch)
    families = plan.block_families(arch, N, torch.float32, True, True, "fp32")
    deferred = plan.bn2_deferred(arch, N, torch.float32, False)
    return SimpleNamespace(arch=arch, N=N, names=names, families=families, deferred=deferred, t_off=arena.t_off,
                           size={p.name: p.size for p in arena.trainable}, arena_floats=arena.n_trainable_padded,
                           fold=plan.fold_layout(arch, names, arena.t_off, N, families), scratch=plan.scratch_floats(arch, N, deferred))


def ceil_div(a, b):
    return -(-a // b)


def wgrad_problems(L, tensor):
    """Every Passes.wgrad_conv call of a backward pass (passes.py), in its order, on tensors of the plan's shapes:
    (x, dy, k, dil, fold key, x_scale)."""
    a, N, out = L.arch, L.N, []
    for j in range(len(a.rsd) - 1, -1, -1):
        m, h, co = a.rsd[j], a.rsd[j].h, a.rsd[j].c_out
        (k0, _, _), (k1, _, _), (kf, _, _) = L.names.n_rsd[j]
        cat, dpyr, tail = tensor(N, h, h, m.c_cat), tensor(N, h, h, 2 * co), L.fold.filter_tail[j]
        out.append((tensor(N, h, h, 2 * co), tensor(N, h, h, co), 3, 1, kf, None))
        for dz, kname, kk, dil in ((dpyr[..., :co], k0, 1, 1), (dpyr[..., co:], k1, 3, 2)):
            out.append((cat[..., :m.c_cat - tail], dz, kk, dil, kname, None))
            if tail:
                out.append((cat[..., m.c_cat - tail:], dz, kk, dil, kname + "#tail", None))
        if m.upsample_conv:
            out.append((cat[..., :m.c_deep], tensor(N, h, h, co), 1, 1, L.names.n_rsd_up[j][0], None))
    ex = a.executed()
    if a.skipdec is not None:
        sd, h = a.skipdec, a.skipdec.h
        (k0, _), seps = L.names.n_skipdec
        for cin, (_, _, pwn, _) in ((sd.c_sep, seps[1]), (sd.c_cat, seps[0])):
            out.append((tensor(N, h, h, cin), tensor(N, h, h, sd.c_sep), 1, 1, pwn, None))
        out.append((tensor(N, h, h, sd.c_skip_in), tensor(N, h, h, sd.c_skip), 1, 1, k0, None))
    for b, nm in reversed(list(zip(ex, L.names.n_blocks))):
        out.append((tensor(N, b.h_out, b.h_out, b.cexp), tensor(N, b.h_out, b.h_out, b.cout), 1, 1, nm["w_proj"], tensor(N, b.cexp)))
        if b.expand != 1:
            out.append((tensor(N, b.h_in, b.h_in, b.cin), tensor(N, b.h_in, b.h_in, b.cexp), 1, 1, nm["w_exp"], None))
    return out


def shape_of(x, dy, k):
    return dy.shape[0], dy.shape[1], dy.shape[2], x.shape[3], dy.shape[3], k


@pytest.mark.parametrize("case", list(CASES))
def test_fold_rows_write_every_gradient_element_at_most_once(case):
    """Row (off, out, total, seg_len, seg_stride, seg_off, nblk, tile) writes the arena elements out + seg_off + (i // seg_len) *
    seg_stride + i % seg_len, i < total.  No element twice, none outside the tensor the row names, and a tensor that has rows is
    covered whole -- but for the RSD fuse conv, whose pooled third of the input channels (rows [2 c_out, c_pyr) of every tap) is the
    share ops.rsd_pool_bwd writes itself: there the rows cover exactly the convolved rows [0, 2 c_out)."""
    L = layout(case)
    fold, a = L.fold, L.arch
    hits = np.zeros(L.arena_floats, dtype=np.int32)
    assert len(fold.regions) == len(fold.rows)
    named = set()
    for key, (off, out, total, seg_len, seg_stride, seg_off, nblk, tile) in zip(fold.regions, fold.rows):
        name = key.split("#")[0]
        named.add(name)
        i = np.arange(total, dtype=np.int64)
        e = out + seg_off + (i // seg_len) * seg_stride + i % seg_len
        assert out == L.t_off[name] and e.min() >= out and e.max() < out + L.size[name], key
        np.add.at(hits, e, 1)
    assert hits.max() == 1
    fuse = {nm[2][0]: m for m, nm in zip(a.rsd, L.names.n_rsd)}
    for name in named:
        got = hits[L.t_off[name]:L.t_off[name] + L.size[name]]
        if name in fuse:
            m = fuse[name]
            assert (got.reshape(9, m.c_pyr, m.c_out)[:, :2 * m.c_out] == 1).all() and not got.reshape(9, m.c_pyr, m.c_out)[:, 2 * m.c_out:].any()
        else:
            assert got.sum() == L.size[name], name
    tails = [k for k in fold.regions if k.endswith("#tail")]
    assert len(tails) == 2 * sum(1 for t in fold.filter_tail.values() if t)
    if case == "b0-224-n8":   # (the 136-channel concat of RSD(2) is split; figures of the layout before it was a function)
        assert len(tails) == 2 and len(fold.rows) == 40 and int(hits.sum()) == 1485600 and sum(L.size.values()) == 2071714


@pytest.mark.parametrize("case", list(CASES))
def test_fold_regions_are_disjoint_aligned_and_as_large_as_the_library_asks(case):
    from mliis_amd import ops
    L = layout(case)
    fold, a, N = L.fold, L.arch, L.N
    spans = sorted((off, off + nblk * total) for off, _, total, _, _, _, nblk, _ in fold.rows)
    assert all(off % 4 == 0 for off, _ in spans) and spans[-1][1] <= fold.floats
    assert all(e0 <= b1 for (_, e0), (b1, _) in zip(spans, spans[1:]))
    for (key, (off, floats)), row in zip(fold.regions.items(), fold.rows):
        assert off == row[0] and row[6] >= 1 and row[6] * row[2] <= floats, key
    # the running tile count
    tile, per = 0, ops.fold_tile_outputs()
    for row in fold.rows:
        assert row[7] == tile
        tile += ceil_div(row[2], per)
    assert fold.tiles == tile
    # every region against the library's workspace query for the problem its launch is given: the dense convs from the shapes
    # passes.py calls them with, the rest from the block geometry
    need = {}
    for x, dy, k, _, key, _ in wgrad_problems(L, lambda *s: torch.empty(1).expand(*s)):   # (shapes only: no storage)
        need[key] = ops.conv2d_bwd_filter_floats(*shape_of(x, dy, k))
    need[L.names.n_stem[0]] = ops.stem_conv_bwd_filter_floats(N, a.image_size, a.image_size, a.stem_out)
    for b, nm, (small, march, _) in zip(a.executed(), L.names.n_blocks, L.families):
        if march:
            need[nm["w_dw"]] = ops.dwconv_bn_bwd_blocks(N, b.h_in, b.h_in, b.cexp, b.k, b.stride) * b.k * b.k * b.cexp
        elif not small:
            need[nm["w_dw"]] = ops.dwconv_bwd_filter_floats(N, b.h_in, b.h_in, b.cexp, b.k, b.stride)
        assert small or nm["w_dw"] in fold.regions
    if a.skipdec is not None:
        for cin, (dwn, _, _, _) in zip((a.skipdec.c_cat, a.skipdec.c_sep), L.names.n_skipdec[1]):
            need[dwn] = ops.dwconv_bwd_filter_floats(N, a.skipdec.h, a.skipdec.h, cin, 3, 1)
    for m, nm, up in zip(a.rsd, L.names.n_rsd, L.names.n_rsd_up):
        for bias in [nm[0][1], nm[1][1]] + ([up[1]] if up else []):
            need[bias] = ops.bn_bwd_dxsum_floats(N * m.h * m.h, m.c_out)
    assert set(need) == set(fold.regions)
    for key, n in need.items():
        assert 0 < n <= fold.regions[key][1], key
    if case == "b0-224-n8":
        assert (fold.tiles, fold.floats) == (5815, 27065904)


@pytest.mark.parametrize("case", list(CASES))
def test_squeeze_excite_tiles_are_a_running_sum(case):
    from mliis_amd import plan
    L = layout(case)
    begins, tiles = plan.se_tile_begins(L.arch)
    want = 0
    for b, t in zip(L.arch.executed(), begins):
        assert t == want
        want += ceil_div(2 * b.cexp * b.se + b.cexp + b.se, 256)   # (256 outputs per workgroup: se_wgrad_tile, csrc/se_wgrad.hpp)
    assert tiles == want and len(begins) == len(L.arch.executed())
    if case == "b0-224-n8":
        assert (len(begins), tiles) == (11, 594)


def scratch_bounds(L, deferred):
    """What each launch the passes can route to a scratch buffer may write there: (buffer, floats, launch).  From the library's query
    where it has one; otherwise the launch's block rule as its wrapper states it."""
    from mliis_amd import ops
    a, N, ex = L.arch, L.N, L.arch.executed()
    rule16 = lambda rows, c: ceil_div(rows, 16) * 2 * c   # noqa: E731  (a GEMM epilogue's statistics: ops.conv2d_fwd's own check)
    stats = ops.bn_stats_partial_floats                   # (the statistics kernel: mliis_colreduce_workspace_floats)
    hs, H = a.h_stem, a.image_size
    out = [("stats_part", stats(N * hs * hs, a.stem_out), "stem bn"), ("stats_part", ops.stem_conv_fwd_stats_floats(N, H, H, a.stem_out), "stem conv")]
    for b, (small, march, _), d in zip(ex, L.families, deferred):
        ri, ro, ce, tag = N * b.h_in ** 2, N * b.h_out ** 2, b.cexp, "block {} ".format(b.idx)
        out += [("stats_part", rule16(ri, ce), tag + "expand conv"), ("stats_part", stats(ri, ce), tag + "bn0"),
                ("stats_part", stats(ro, ce), tag + "bn1"), ("stats_part", stats(ro, b.cout), tag + "bn2"),
                ("stats_part", rule16(ro, b.cout), tag + "project conv"),
                # (dwconv_fwd's statistics: a block per 32 strips of an output row, never more than a block per 16 pixels)
                ("stats_part", rule16(ro, ce), tag + "op-by-op depthwise"),
                ("sums_part", ops.se_bn_bwd_sums_floats(N, b.h_out ** 2, ce), tag + "se_bn_bwd_sums"), ("stage1_se", 2 * N * ce, tag + "se_mlp_bwd_bn"),
                ("pool_part", N * ceil_div(b.h_out ** 2, 128) * ce, tag + "bn1 apply pooling")]
        if march:
            geo = (N, b.h_in, b.h_in, ce, b.k, b.stride)
            out += [("stats_part2", ops.dwconv_bn_fwd_blocks(*geo) * 2 * ce, tag + "dwconv_bn_fwd"),
                    ("stats_part2", ops.dwconv_bn_bwd_blocks(*geo) * 2 * ce, tag + "dwconv_bn_bwd")]
        if 16 <= b.h_out ** 2 <= 256:
            out.append(("gate_part", rule16(ro, ce), tag + "project backward-data gate partials"))
        if d:
            out += [("stats_part3", rule16(ro, b.cout), tag + "deferred project conv"), ("stats_part3", stats(ro, b.cout), tag + "deferred bn2")]
    for m in a.rsd:
        rows = N * m.h * m.h
        out += [("stats_part", rule16(rows, m.c_out), "rsd conv"), ("stats_part", stats(rows, m.c_out), "rsd bn"),
                ("stats_part2", rule16(rows, m.c_out), "rsd dilated conv"), ("stats_part2", stats(rows, m.c_out), "rsd dilated bn")]
    if a.skipdec is not None:
        rows = N * a.skipdec.h ** 2
        for c in (a.skipdec.c_skip, a.skipdec.c_cat, a.skipdec.c_sep):
            out += [("stats_part", rule16(rows, c), "skipdec conv"), ("stats_part", stats(rows, c), "skipdec bn")]
    return out


@pytest.mark.parametrize("case", list(CASES) + ["b0-224-n8 fuse_bn2"])
def test_scratch_buffers_hold_what_their_launches_write(case):
    from mliis_amd import plan
    L = layout(case.split()[0])
    deferred, scratch = L.deferred, L.scratch
    if case.endswith("fuse_bn2"):
        deferred = plan.bn2_deferred(L.arch, L.N, torch.float32, True)
        scratch = plan.scratch_floats(L.arch, L.N, deferred)
        assert any(deferred) and not deferred[-1]
    else:
        assert not any(deferred) and scratch["stats_part3"] == 64
    assert set(scratch) == {"stats_part", "stats_part2", "stats_part3", "sums_part", "stage1_se", "pool_part", "gate_part"}
    for name, floats, what in scratch_bounds(L, deferred):
        assert floats <= scratch[name] - 64, (name, what, floats, scratch[name])   # (the 64-float pad is slack, not capacity)
    if case == "b0-224-n8":
        assert scratch == dict(stats_part=1204288, stats_part2=351296, stats_part3=64, sums_part=67264, stage1_se=10816, pool_part=28864,
                               gate_part=131776)


# ---------------------------------------------------------------------------------------------- ops.FilterBatch
def decode(row):
    """A table row as conv_filter_grad2_batched_k reads it (the comment above kFilterDescWords, csrc/conv_gemm_kernels.hpp)."""
    return SimpleNamespace(Cin=row[9], Cout=row[10], k=row[11] & 0xff, multitap=(row[13] >> 32) & 1, gx=row[14] & 0xfffff,
                           gy=(row[14] >> 20) & 0xfffff, gz=row[14] >> 40, first=row[15], slabs=row[3])


@functools.lru_cache(maxsize=None)
def batch(merge_max=None, wide=None):
    """FilterBatch over the 29 filter-gradient problems of b0, 224, N = 8 on CPU tensors; returns (batch, problems, floats of the
    fold region at a slab address)."""
    from mliis_amd import ops
    L = layout("b0-224-n8")
    fold_buf = torch.empty(L.fold.floats)
    probs = wgrad_problems(L, lambda *s: torch.empty(s))
    fb = ops.FilterBatch(torch.device("cpu"))
    if merge_max is not None:
        fb.MERGE_MAX_BLOCKS = merge_max
    if wide is not None:
        fb.X3_WIDE = wide
    region = {}
    for x, dy, k, dil, key, sc in probs:
        o, n = L.fold.regions[key]
        fb.add(x, dy, k, dil, fold_buf[o:o + n], x_scale=sc)
        region[fold_buf[o:o + n].data_ptr()] = n
    fb._build()
    return fb, probs, region


def check_tables(fb, region):
    """Every table, narrow and wide: the problems' block ranges tile the grid, and no re-tiling changes what a problem needs of its
    slab region."""
    for t in fb.tables:
        for table, blocks in [(t.table, t.blocks)] + ([tuple(t.wide)] if t.wide is not None else []):
            rows = [decode(r) for r in table.tolist()]
            assert len(rows) == t.nprob <= 64
            first = 0
            for p in rows:
                assert p.first == first
                first += p.gx * p.gy * p.gz
                assert p.gz * p.k * p.k * p.Cin * p.Cout <= region[p.slabs]
            assert first == blocks
        if t.wide is not None:
            assert [decode(r).gz for r in t.wide.table.tolist()] == [decode(r).gz for r in t.table.tolist()]


def native_plan(x, dy, k):
    """(tmf, nt, multitap, gx, gy, gz, rows_per_split) of mliis_conv2d_bwd_filter_plan."""
    import ctypes as C
    from mliis_amd import ops
    plan = (C.c_int * 8)()
    ops.lib.call("mliis_conv2d_bwd_filter_plan", *shape_of(x, dy, k), plan)
    return [int(v) for v in plan[:7]]


def test_filter_batch_tables_of_b0():
    fb, probs, region = batch()
    assert len(probs) == len(fb) == 29
    check_tables(fb, region)
    assert [(t.nprob, t.blocks, t.tmf, t.nt, t.has_scale) for t in fb.tables] == [(15, 3868, 1, 4, 0), (11, 1757, 1, 4, 1), (1, 392, 2, 2, 0),
                                                                                  (2, 1008, 2, 7, 0)]
    assert [t.wide is not None for t in fb.tables] == [False, False, False, True] and fb.tables[3].wide.blocks == 756
    # the fields in the positional order the GPU tests and tools read them in
    t = fb.tables[3]
    assert (t[0] is t.table, t[1], t[2], t[3], t[4], t[5], t[6][0] is t.wide.table, t[6][1]) == (True, 2, 1008, 2, 7, 0, True, 756)
    # pixel splits as the library planned them, whatever was re-tiled
    native = {slab.data_ptr(): native_plan(x, dy, k) for (x, dy, k, _, _, _), slab in zip(probs, fb._keep[2::4])}
    for t in fb.tables:
        for r in t.table.tolist():
            p, (tmf, nt, multitap, gx, gy, gz, _) = decode(r), native[r[3]]
            assert (p.gz, p.multitap) == (gz, multitap)
            if (t.tmf, t.nt) == (1, 4):   # the merged group: 64 columns per workgroup
                assert p.gy == ceil_div(p.Cout, 64) and p.gx == gx and tmf == 1
            else:
                assert (p.gx, p.gy, tmf, nt) == (gx, gy, t.tmf, t.nt)
        if t.wide is not None:
            for r, r0 in zip(t.wide.table.tolist(), t.table.tolist()):
                p, p0 = decode(r), decode(r0)
                assert p.gy == p0.gy and p.gx == (p.k * p.k * ceil_div(p.Cin, 256) if p.Cin > 128 and not p.multitap else p0.gx)


def test_filter_batch_without_merging_and_without_the_wide_form():
    fb, probs, region = batch(merge_max=0)
    check_tables(fb, region)
    groups = {tuple(native_plan(x, dy, k)[:2]) + (int(sc is not None),) for x, dy, k, _, _, sc in probs}
    assert [(t.tmf, t.nt, t.has_scale) for t in fb.tables] == sorted(groups) and len(groups) == 8
    fb, _, region = batch(wide=False)
    check_tables(fb, region)
    assert len(fb.tables) == 4 and all(t.wide is None for t in fb.tables)
