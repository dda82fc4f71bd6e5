"""The buffers of one inner step: every activation, gradient, statistics and scratch tensor of a fixed batch size N, allocated once in
HBM (`_Plan`), plus the launch tables that are built once per plan (deferred filter gradients, slab folds, SE weight gradients, the
mask draws) and the captured HIP graphs of the step.  Which kernel family runs a block (row-marching / small-map fused / op by op) is
decided here, from the C library's own eligibility queries.

The decisions, the scratch sizes and the table layouts are pure functions of (arch, N, flags): integers and names in, integers out,
nothing allocated (tests/test_plan_layout_cpu.py checks them without a GPU).  `_Plan` allocates what they describe."""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops, spec
from ._lib import MliisError


# variable names (TF scopes of the reference model) per layer of an architecture
LayerNames = namedtuple("LayerNames", "n_stem n_blocks n_rsd n_rsd_up n_skipdec n_final n_aspp")


def layer_names(arch) -> LayerNames:
    fe = arch.name
    n_blocks = []
    for b in arch.executed():
        s = f"{fe}/blocks_{b.idx}"
        bns = [f"{s}/tpu_batch_normalization", f"{s}/tpu_batch_normalization_1", f"{s}/tpu_batch_normalization_2"]
        cvs = [f"{s}/conv2d/kernel", f"{s}/conv2d_1/kernel"]
        d = {}
        if b.expand != 1:
            d["w_exp"], d["bn0"] = cvs.pop(0), bns.pop(0)
        d["w_dw"], d["bn1"] = f"{s}/depthwise_conv2d/depthwise_kernel", bns.pop(0)
        d["se"] = (f"{s}/se/conv2d/kernel", f"{s}/se/conv2d/bias", f"{s}/se/conv2d_1/kernel", f"{s}/se/conv2d_1/bias")
        d["w_proj"], d["bn2"] = cvs.pop(0), bns.pop(0)
        n_blocks.append(d)
    n_rsd, n_rsd_up = [], []
    for m in arch.rsd:
        s = f"decode/decode_skip_connections_{m.scope_index}"
        sfx = ["", "_1", "_2", "_3"]
        trip = lambda x: (f"{s}/conv2d{x}/kernel", f"{s}/conv2d{x}/bias", f"{s}/batch_normalization{x}")   # noqa: E731
        n_rsd_up.append(trip(sfx.pop(0)) if m.upsample_conv else None)   # (created first in the scope, efficientlab.py:213-215)
        n_rsd.append([trip(sfx.pop(0)) for _ in range(3)])
    s = "decode/decode_skip_connections"   # --skip_decoding: (1x1 kernel, its BN), then per sep_conv (dw kernel, BN, 1x1 kernel, BN)
    n_skipdec = ((f"{s}/conv2d/kernel", f"{s}/batch_normalization"),
                 [(f"{s}/depthwise_conv2d{'' if j == 0 else '_%d' % j}/depthwise_kernel", f"{s}/batch_normalization_{2 * j + 1}",
                   f"{s}/conv2d_{j + 1}/kernel", f"{s}/batch_normalization_{2 * j + 2}") for j in range(2)])
    s = "decode/spatial_pyramid_pooling"
    return LayerNames((f"{fe}/stem/conv2d/kernel", f"{fe}/stem/tpu_batch_normalization"), n_blocks, n_rsd, n_rsd_up, n_skipdec,
                      ("decode/final_layer_weights/kernel", "decode/final_layer_weights/bias"),
                      [(f"{sc}/conv2d/kernel", f"{sc}/conv2d/bias") for sc in (f"{s}/branch_0", f"{s}/branch_1", f"{s}/branch_2", s)])


def block_families(arch, N, act_dtype, small_fused, dw_march, matmul_precision):
    """Per executed block (small, march, blk): the kernel family of its depthwise half, and the group width of the group-blocked
    layout its 1x1 convs write beside the small-map launches (0: none)."""
    out = []
    for b in arch.executed():
        hi, ho, ce = b.h_in, b.h_out, b.cexp
        # small maps (14x14 at 224x224 inputs): the depthwise half of the block runs as ONE launch per direction (mbconv_small.hip)
        small = bool(small_fused and b.expand != 1 and ops.mbconv_dw_small_supported(N, hi, hi, ce, b.k, b.stride))
        # every other block: the row-marching kernels (batch norm + swish in front of the depthwise conv applied while its input is
        # staged; one-pass backward).  A shape neither family takes (>= 2 GiB tensors, other k / stride) runs op by op (dwconv.hip)
        march = bool(dw_march and not small and ops.dwconv_bn_supported(N, hi, hi, ce, b.k, b.stride))
        if act_dtype != torch.float32 and not (march or small):
            raise MliisError("bf16 storage: block {} ({}x{}x{}, k {}, stride {}) is taken by neither fused depthwise family".format(
                b.idx, hi, hi, ce, b.k, b.stride))
        # fp32 storage and both 1x1 convs beside the fused launches on the streamed plan: they WRITE the group-blocked layout
        # themselves (z0 by the expand conv: no copy; da2 by the project conv's backward-data) -- every access of the fused
        # launches to the expanded tensors but a1 / dz0 is then contiguous
        blocked = (small and act_dtype == torch.float32 and ops.conv1x1_stream_eligible(N, hi, hi, b.cin, ce, matmul_precision)
                   and ops.conv1x1_stream_eligible(N, ho, ho, b.cout, ce, matmul_precision) and 16 <= ho * ho <= 256)
        out.append((small, march, ops.mbconv_dw_small_group_width(ce, b.k) if blocked else 0))
    return out


def bn2_deferred(arch, N, act_dtype, fuse_bn2):
    """Per executed block i: its project batch norm (+ drop-connect, + identity skip) is applied by block i + 1's expand conv while
    it loads its rows (ops.conv2d_fwd_bnin; training passes -- inference keeps the stand-alone apply)."""
    ex = arch.executed()
    return [bool(fuse_bn2 and i + 1 < len(ex) and ex[i + 1].expand != 1 and act_dtype in (torch.float32, torch.bfloat16) and
                 ops.conv2d_fwd_bnin_ok(N, b.h_out, b.h_out, b.cout, ex[i + 1].cexp)) for i, b in enumerate(ex)]


def _stage1_floats(rows, c):
    """Stage-1 batch-norm sums [blocks][2][c] over a [rows, c] tensor, whichever producer leaves them: a GEMM epilogue (a block per 16
    rows) or the statistics kernel."""
    return max(-(-rows // 16) * 2 * c, ops.bn_stats_partial_floats(rows, c))


def scratch_floats(arch, N, deferred):
    """Floats of the step's shared scratch buffers (each with a 64-float pad), sized for the largest launch that writes them.
    deferred: bn2_deferred(...)."""
    a, ex, H, hs = arch, arch.executed(), arch.image_size, arch.h_stem
    # stage-1 BN statistics handed from a producer (GEMM epilogue / stats kernel) to the fused fold+apply kernel
    shapes = [s for b in ex for s in ((N * b.h_in ** 2, b.cexp), (N * b.h_out ** 2, b.cexp), (N * b.h_out ** 2, b.cout))]
    shapes += [(N * m.h * m.h, m.c_out) for m in a.rsd]
    if a.skipdec is not None:
        shapes += [(N * a.skipdec.h ** 2, c) for c in (a.skipdec.c_skip, a.skipdec.c_cat, a.skipdec.c_sep)]
    stats = max([_stage1_floats(rows, c) for rows, c in shapes] +
                [ops.bn_stats_partial_floats(N * hs * hs, a.stem_out), ops.stem_conv_fwd_stats_floats(N, H, H, a.stem_out)])
    # the row-marching depthwise kernels (ops.dwconv_bn_fwd / _bwd) READ the producer's partial sums from stats_part while other
    # workgroups of the same launch already WRITE theirs: a second buffer
    # (and the second RSD branch GEMM's statistics, folded together with the first's by ops.bn_apply_fused_pair)
    stats2 = max([blocks(N, b.h_in, b.h_in, b.cexp, b.k, b.stride) * 2 * b.cexp
                  for b in ex for blocks in (ops.dwconv_bn_fwd_blocks, ops.dwconv_bn_bwd_blocks)] +
                 [_stage1_floats(N * m.h * m.h, m.c_out) for m in a.rsd] + [0])
    # project-BN-on-load (ops.conv2d_fwd_bnin): block i's project conv leaves its statistics in a THIRD buffer -- block i + 1's expand
    # conv folds them while its own workgroups already write the next batch norm's into stats_part
    stats3 = max([-(-(N * b.h_out ** 2) // 16) * 2 * b.cout for b, d in zip(ex, deferred) if d] + [0])
    return dict(
        stats_part=stats + 64, stats_part2=stats2 + 64, stats_part3=stats3 + 64,
        # the squeeze-excite backward and the depthwise batch norm's backward share ONE pass over (da2, z1) (ops.se_bn_bwd_sums): its
        # per-image chunk sums, and the batch norm's stage-1 sums per image that ops.se_mlp_bwd_bn forms from them
        sums_part=max([ops.se_bn_bwd_sums_floats(N, b.h_out * b.h_out, b.cexp) for b in ex] + [0]) + 64,
        stage1_se=max([2 * N * b.cexp for b in ex] + [0]) + 64,
        # squeeze-excite pooling partials of the bn1 apply pass: [N][ceil(rows_per_img / 128)][C]
        pool_part=max(N * (-(-(b.h_out * b.h_out) // 128)) * b.cexp for b in ex) + 64,
        # gate-gradient partials of the project backward-data launch on the small maps: [16-row groups][2][C]
        gate_part=max([(-(-(N * b.h_out * b.h_out) // 16)) * 2 * b.cexp for b in ex if 16 <= b.h_out * b.h_out <= 256] + [0]) + 64)


# The deferred weight-gradient folds: every *_bwd_filter leaves its per-split slabs in a region of fold_buf and ONE mliis_fold_batched
# launch at the end of the backward pass reduces them all into the gradient arena.  regions: key (a variable name, or name + "#tail") ->
# (offset, floats) in fold_buf; rows: [n][8] {offset, arena offset, total, seg_len, seg_stride, seg_off, slabs, first tile}
# (include/mliis_hip.h); floats: size of fold_buf; filter_tail: RSD module -> channels of the concat's sliver with a region of its own
FoldLayout = namedtuple("FoldLayout", "regions rows tiles floats filter_tail")


def fold_layout(arch, names, t_off, N, families) -> FoldLayout:
    a, H = arch, arch.image_size
    regs, rows, filter_tail, off, tile = {}, [], {}, 0, 0
    fold_tile = ops.fold_tile_outputs()
    conv, dwconv = ops.conv2d_bwd_filter_floats, ops.dwconv_bwd_filter_floats

    def add(name, ws_floats, total, seg=None, key=None):
        nonlocal off, tile
        seg_len, seg_stride, seg_off = seg or (total, 0, 0)
        regs[key or name] = (off, ws_floats)
        rows.append([off, t_off[name], total, seg_len, seg_stride, seg_off, ws_floats // total, tile])
        off += (ws_floats + 3) // 4 * 4
        tile += -(-total // fold_tile)
    add(names.n_stem[0], ops.stem_conv_bwd_filter_floats(N, H, H, a.stem_out), 27 * a.stem_out)
    for b, nm, (small, march, _) in zip(a.executed(), names.n_blocks, families):
        ce = b.cexp
        if b.expand != 1:
            add(nm["w_exp"], conv(N, b.h_in, b.h_in, b.cin, ce, 1), b.cin * ce)
        if march:
            add(nm["w_dw"], ops.dwconv_bn_bwd_blocks(N, b.h_in, b.h_in, ce, b.k, b.stride) * b.k * b.k * ce, b.k * b.k * ce)
        elif not small:   # (the small-map backward kernel writes the complete depthwise filter gradient itself: no slabs)
            add(nm["w_dw"], dwconv(N, b.h_in, b.h_in, ce, b.k, b.stride), b.k * b.k * ce)
        add(nm["w_proj"], conv(N, b.h_out, b.h_out, ce, b.cout, 1), ce * b.cout)
    if a.skipdec is not None:
        sd, h = a.skipdec, a.skipdec.h
        ksk, seps = names.n_skipdec
        add(ksk[0], conv(N, h, h, sd.c_skip_in, sd.c_skip, 1), sd.c_skip_in * sd.c_skip)
        cin = sd.c_cat
        for (dwn, _, pwn, _) in seps:
            add(dwn, dwconv(N, h, h, cin, 3, 1), 9 * cin)
            add(pwn, conv(N, h, h, cin, sd.c_sep, 1), cin * sd.c_sep)
            cin = sd.c_sep
    for j, (m, nm) in enumerate(zip(a.rsd, names.n_rsd)):
        (k0, b0, _), (k1, b1, _), (kf, _, _) = nm
        co, h = m.c_out, m.h
        if m.upsample_conv:
            ku, bu, _ = names.n_rsd_up[j]
            add(ku, conv(N, h, h, m.c_deep, co, 1), m.c_deep * co)
            add(bu, ops.bn_bwd_dxsum_floats(N * h * h, co), co)
        for bias in (b0, b1):   # conv-bias gradients: column sums of dz leave the BN backward pass as slabs
            add(bias, ops.bn_bwd_dxsum_floats(N * h * h, co), co)
        # filter gradients over the concatenated [deep | skip] channels.  A channel count like 136 = 2 * 64 + 8 leaves a third of
        # the 64-channel blocks of the filter-gradient kernel nearly empty while they still occupy a CU slot each: the sliver
        # (c_cat mod 64 <= 16 channels) gets its own small launch and fold region instead (profiles/r01_notes.md).
        tail = filter_tail[j] = m.c_cat % 64 if (m.c_cat > 64 and 0 < m.c_cat % 64 <= 16) else 0
        main_c = m.c_cat - tail
        for kk, kname in ((1, k0), (3, k1)):
            add(kname, conv(N, h, h, main_c, co, kk), kk * kk * main_c * co, seg=(main_c * co, m.c_cat * co, 0) if tail else None)
            if tail:
                add(kname, conv(N, h, h, tail, co, kk), kk * kk * tail * co, seg=(tail * co, m.c_cat * co, main_c * co), key=kname + "#tail")
        add(kf, conv(N, h, h, 2 * co, co, 3), 9 * 2 * co * co, seg=(2 * co * co, m.c_pyr * co, 0))
    return FoldLayout(regs, rows, tile, off + 16, filter_tail)


SE_WGRAD_TILE = 256   # weight-gradient outputs per workgroup of the batched squeeze-excite launch (se_wgrad_tile, csrc/se_wgrad.hpp)


def se_tile_begins(arch):
    """First tile of every executed block in the squeeze-excite weight-gradient launch (a tile: SE_WGRAD_TILE of the block's
    2 C R + C + R outputs), and the launch's tile count."""
    begins, tile = [], 0
    for b in arch.executed():
        begins.append(tile)
        tile += -(-(2 * b.cexp * b.se + b.cexp + b.se) // SE_WGRAD_TILE)
    return begins, tile


class _Plan:
    """All activation / gradient buffers of one inner step for a fixed batch size N."""

    def __init__(self, L: "Learner", N: int, act_dtype=torch.float32):
        a, dev, A = L.arch, L.device, L.arena
        self.N = N
        # storage type of the EXPANDED tensors of the MBConv blocks (z0, z1, a1, da2, da0 / dz0): fp32, or bf16 for the training plan of
        # `--precision bf16-storage` (BASELINE configs[3]).  Everything else -- block inputs / outputs, the decoder, statistics, sums,
        # parameters -- is fp32 in every mode.
        self.act_dtype = act_dtype
        # ---- 1. decisions
        families = block_families(a, N, act_dtype, L.small_fused, L.dw_march, L.matmul_precision)
        self.bn2_deferred = bn2_deferred(a, N, act_dtype, L.fuse_bn2)
        # block 0 without an expand conv (EfficientNet-B0 ... B7) takes the stem's BN + swish into its depthwise launch: the activated
        # stem output is only read there (no identity skip), so it is never written
        ex = a.executed()
        self.fuse_stem = bool(ex and families[0][1] and ex[0].expand == 1 and not ex[0].skip)
        # ---- 2. activations and gradients
        self._alloc_activations(L, families)
        # ---- 3. scratch shared by the launches of a step
        for name, floats in scratch_floats(a, N, self.bn2_deferred).items():
            setattr(self, name, torch.empty(floats, dtype=torch.float32, device=dev))
        # ---- 4. launch tables.  Squeeze-excite weight gradients of all blocks: one launch (descriptor table of device addresses)
        names = layer_names(a)
        begins, self.se_tiles = se_tile_begins(a)
        self.se_desc = torch.tensor([[B[k].data_ptr() for k in ("s", "hpre", "dpre1", "dpre2")] + [A.g[k].data_ptr() for k in nm["se"]] +
                                     [N, b.cexp, b.se, t] for b, B, nm, t in zip(ex, self.blocks, names.n_blocks, begins)],
                                    dtype=torch.int64, device=dev)
        fold = fold_layout(a, names, A.t_off, N, families)
        self.filter_tail = fold.filter_tail
        self.fold_buf = torch.empty(fold.floats, dtype=torch.float32, device=dev)
        self.fold_part = {k: self.fold_buf[o:o + n] for k, (o, n) in fold.regions.items()}
        self.fold_desc = torch.tensor(fold.rows, dtype=torch.int64, device=dev)
        self.fold_tiles = fold.tiles
        # ---- 5. captured hipGraphExecs of the training step: key True = the step draws its masks on the device (mliis_rng_masks inside
        # the graph), False = masks were handed in by the caller (parity tests inject them) and the graph starts after them
        self.graphs = {}
        self.steps_run = 0
        # deferred dense-conv filter gradients: collected during the first (eager) backward pass of this plan, then one launch per
        # kernel instantiation at the end of every backward pass (ops.FilterBatch)
        self.wbatch = ops.FilterBatch(dev)
        self.wbatch_ready = False
        # mask generation inside the step (ops.rng_masks): drop-connect scales of all skip blocks, final-layer dropout, ASPP dropouts
        jobs = []
        if L.drop_connect and any(b.skip for b in ex):
            jobs.append((self.dc_all, L._dc_keeps, N, True))
        if self.drop_mask is not None:
            jobs.append((self.drop_mask, L.drop_keep_dev, self.drop_mask.numel(), False))
        if self.aspp is not None:
            for mbuf in self.aspp["masks"]:
                jobs.append((mbuf, 1.0 - spec.ASPP_DROPOUT, 1, False))
        self.mask_plan = ops.MaskPlan(jobs) if jobs else None

    def _alloc_activations(self, L, families):
        a, dev, N, act_dtype = L.arch, L.device, self.N, self.act_dtype

        def buf(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        def xbuf(*shape):
            return torch.empty(shape, dtype=act_dtype, device=dev)

        def vec(c):
            return buf(c), buf(c)
        self.idx = torch.zeros(N, dtype=torch.int32, device=dev)
        H = a.image_size
        hs = a.h_stem
        self.z_stem, self.st_stem = buf(N, hs, hs, a.stem_out), vec(a.stem_out)
        self.a_stem = None if self.fuse_stem else buf(N, hs, hs, a.stem_out)
        self.blocks = []
        nskip = sum(1 for b in a.executed() if b.skip)
        self.dc_all = torch.ones(max(nskip, 1), N, dtype=torch.float32, device=dev)
        si = 0
        for b, (small, march, blk) in zip(a.executed(), families):
            B = dict(small=small, march=march, blk=blk)
            hi, ho, ce = b.h_in, b.h_out, b.cexp
            if b.expand != 1:
                B["z0"], B["st0"] = xbuf(N, hi, hi, ce), vec(ce)
                if not march:   # (the marching kernels apply bn0 + swish on load: a0 is never written; small-map blocks run op by op in inference)
                    B["a0"] = xbuf(N, hi, hi, ce)
            B["z1"], B["a1"], B["st1"] = xbuf(N, ho, ho, ce), xbuf(N, ho, ho, ce), vec(ce)
            if small:   # the fused small-map kernels save z0 (a copy) and z1 in their group-blocked layout for the backward launch
                B["z0b"] = xbuf(N, hi, hi, ce)
            B["s"], B["hpre"], B["gate"] = buf(N, ce), buf(N, b.se), buf(N, ce)
            B["z2"], B["st2"], B["out"] = buf(N, ho, ho, b.cout), vec(b.cout), buf(N, ho, ho, b.cout)
            B["dout"] = buf(N, ho, ho, b.cout)
            B["dgate"], B["dpre1"], B["dpre2"], B["chan_add"] = buf(N, ce), buf(N, b.se), buf(N, ce), buf(N, ce)
            if b.skip:
                B["dc"] = self.dc_all[si]
                si += 1
            # gradients w.r.t. the expanded activations: one pair PER BLOCK (not a shared scratch) so the weight-gradient kernels of a
            # block can run on the side stream while the main stream already works on the next block
            B["da2"] = xbuf(N, ho, ho, ce)
            # (a block without an expand conv: the depthwise backward's output is the gradient of the block's fp32 input)
            B["da0"] = xbuf(N, hi, hi, ce) if b.expand != 1 else buf(N, hi, hi, ce)
            self.blocks.append(B)
        self.dstem = buf(N, hs, hs, a.stem_out)
        self.rsd = []
        for m in a.rsd:
            D = {}
            h = m.h
            D["cat"] = buf(N, h, h, m.c_cat)
            D["z0"], D["z1"], D["zf"] = buf(N, h, h, m.c_out), buf(N, h, h, m.c_out), buf(N, h, h, m.c_out)
            D["st0"], D["st1"], D["stf"] = vec(m.c_out), vec(m.c_out), vec(m.c_out)
            D["pyr"] = buf(N, h, h, 2 * m.c_out)        # the pooled third of the reference's "pyramid" is never materialised
            D["pool"], D["dpool"] = buf(N, m.c_cat), buf(N, m.c_cat)
            D["pool_part"] = buf(max(1, ops.rsd_concat_pool_floats(N, h, h, m.c_cat)))
            D["bbias"], D["tot"] = buf(N, 9, m.c_out), buf(N, m.c_out)
            D["out"], D["dout"] = buf(N, h, h, m.c_out), buf(N, h, h, m.c_out)
            D["dzf"], D["dpyr"], D["dcat"] = buf(N, h, h, m.c_out), buf(N, h, h, 2 * m.c_out), buf(N, h, h, m.c_cat)
            if m.upsample_conv:   # the residual operand's own 1x1 branch (efficientlab.py:213-215), deep channels != c_out
                D["zu"], D["stu"], D["up2"] = buf(N, h, h, m.c_out), vec(m.c_out), buf(N, h, h, m.c_out)
                D["dzu"], D["dup"] = buf(N, h, h, m.c_out), buf(N, h, h, m.c_deep)
            self.rsd.append(D)
        self.skipdec = None
        if a.skipdec is not None:   # --skip_decoding (efficientlab.py:133-149)
            sd, h = a.skipdec, a.skipdec.h
            T = dict(cat=buf(N, h, h, sd.c_cat), dcat=None, z0=buf(N, h, h, sd.c_skip), st0=vec(sd.c_skip), dz0=buf(N, h, h, sd.c_skip),
                     dout=buf(N, h, h, sd.c_sep), sep=[])
            cin = sd.c_cat
            for _ in range(2):
                T["sep"].append(dict(zd=buf(N, h, h, cin), std=vec(cin), ad=buf(N, h, h, cin), zp=buf(N, h, h, sd.c_sep), stp=vec(sd.c_sep),
                                     out=buf(N, h, h, sd.c_sep), dad=buf(N, h, h, cin), din=buf(N, h, h, cin)))
                cin = sd.c_sep
            self.skipdec = T
        self.aspp = None
        if a.aspp:   # --spatial_pyramid_pooling (models/efficientlab.py:248-289)
            h, ci, d = a.aspp_h, a.aspp_cin, a.aspp_dimension
            self.aspp = dict(z0=buf(N, h, h, d), z1=buf(N, h, h, d), cat=buf(N, h, h, 3 * d), dcat=buf(N, h, h, 3 * d), zo=buf(N, h, h, d),
                             out=buf(N, h, h, d), dout=buf(N, h, h, d), dzo=buf(N, h, h, d), pool=buf(N, ci), dpool=buf(N, ci),
                             z2=buf(N, d), b2=buf(N, d), db2=buf(N, d),
                             masks=[buf(N, h, h, d), buf(N, h, h, d), buf(N, d), buf(N, h, h, d)])
        hd = a.h_dec
        self.small, self.dsmall = buf(N, hd, hd, 2), buf(N, hd, hd, 2)
        self.logits, self.dlogits, self.pred = buf(N, H, H, 2), buf(N, H, H, 2), buf(N, H, H, 2)
        self.drop_mask = buf(N, hd, hd, a.c_final) if L.final_layer_dropout_rate > 0 else None
        self.loss_out = torch.zeros(4, dtype=torch.float32, device=dev)
        # the fused head launch's workspace (the first step that takes it allocates it) and its hand-over to the final conv's backward-data
        self.head_ws = self.head_fin = None
        # Learner.score_resident: the [N,4] IoU counts on the device and their pinned host copy (allocated by the first scoring call)
        self.counts = self.counts_pin = None
        # Learner.mask_resident: the [N,words] bit-packed masks on the device and their pinned host copy (allocated by its first call)
        self.bits = self.bits_pin = None
        # Learner.histogram_resident: the [N,2,256] probability histograms on the device and their pinned host copy (allocated by its
        # first call; with masks=True it packs into the buffers above)
        self.hist = self.hist_pin = None
        # Learner._forward_views (views= of the scoring calls): the mirrored batch [N,H,H,3] and the sum of the mirrored views'
        # decoder-resolution logits [N,hd,hd,2] (allocated by the first call with a view; never without one)
        self.view_x = self.view_acc = None

    @property
    def graph(self):
        """Any captured graph of this plan (None: none yet)."""
        for g in self.graphs.values():
            return g
        return None
