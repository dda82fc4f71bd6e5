"""The two passes of an inner step as launch sequences over a plan's buffers (`_Plan`, plan.py): forward (stem -> MBConv blocks ->
[ASPP | DeepLabv3+-style decoder] -> residual skip decoders -> head) and backward, each a fixed sequence of C-ABI kernel launches
(ops.py) -- no torch op, no host decision that depends on data.  A mixin of `Learner` (learner.py), which owns the weights (arena),
the streams, graph capture and the checkpoint / meta-learner interface.  `_forward` and `_backward` name the stages in order and hand
the values between them; the launches of one stage (stem, an MBConv family, a decoder) are one method over the helpers of `_Pass`.

Graph semantics restated from: models/efficientlab.py:111-119,126-231,248-289,294-317; models/efficientnet/efficientnet_model.py:
175-290,396-441; models/efficientnet/utils.py:87-170.  Backward formulas: SURVEY.md Appendix B."""
from __future__ import annotations

import torch

from . import ops, spec
from ._lib import MliisError
from .plan import _Plan


class _Pass:
    """One pass over a plan: the learner, the plan, the mode, and the launches every stage shares."""

    def __init__(self, L, P: _Plan, training: bool, stochastic: bool = True):
        self.L, self.P, self.training = L, P, training
        self.stochastic = training and stochastic   # drop-connect / dropout masks are applied (a training step; predict() never)
        self.w, self.mv, self.g, self.ws = L.arena.w, L.arena.mv, L.arena.g, L.ws

    def moving(self, prefix):
        return self.mv[prefix + "/moving_mean"], self.mv[prefix + "/moving_variance"]

    def bn_bwd_args(self, st, prefix):
        """(mean, rstd, gamma, beta): the order of the backward kernels (and of the stand-alone apply kernels)."""
        return st[0], st[1], self.w[prefix + "/gamma"], self.w[prefix + "/beta"]

    def bn_fwd_args(self, st, prefix, moving=True):
        """(gamma, beta, mean, rstd, moving_mean, moving_variance): the order of the fused depthwise forward kernels.
        moving=False: (..., None, None) -- mean / rstd are inputs, no moving average is updated."""
        return (self.w[prefix + "/gamma"], self.w[prefix + "/beta"], st[0], st[1]) + (self.moving(prefix) if moving else (None, None))

    def moving_stats(self, st, prefix):
        """Inference: the moving statistics as the batch norm's mean / rstd."""
        mean, var = self.moving(prefix)
        st[0].copy_(mean)
        torch.rsqrt(var + spec.BN_EPS, out=st[1])

    def bn(self, xin, st, prefix, y, pre=False, post=False, img_scale=None, res=None, fused=False, nblk=0, pool_part=None, always_batch=False,
           part=None):
        """nblk > 0: the producing conv already left the stage-1 statistics in P.stats_part.  always_batch: a batch norm the
        reference builds with training=True (the --skip_decoding decoder): batch statistics in inference too, moving averages
        untouched there."""
        P = self.P
        if self.training or always_batch:
            part = P.stats_part if (part is None or nblk == 0) else part
            if nblk == 0:
                nblk = ops.bn_stats_partial(xin, pre, P.stats_part)
            return ops.bn_apply_fused(xin, part, nblk, *self.bn_bwd_args(st, prefix), moving=self.moving(prefix) if self.training else None,
                                      unbiased_moving_var=fused, pre_swish=pre, post_swish=post, img_scale=img_scale, res=res, out=y,
                                      pool_part=pool_part)
        self.moving_stats(st, prefix)
        return ops.bn_apply(xin, *self.bn_bwd_args(st, prefix), pre, post, img_scale, res, out=y)

    def bn_in(self, z, st, prefix, nblk):
        """The batch norm in front of a marching depthwise launch: (bn tuple, nblk) for ops.dwconv_bn_fwd.  Training: the launch
        folds the producer's partial sums (P.stats_part) and updates the moving averages; inference: moving statistics given."""
        if self.training:
            if nblk == 0:
                nblk = ops.bn_stats_partial(z, False, self.P.stats_part)
            return self.bn_fwd_args(st, prefix), nblk
        self.moving_stats(st, prefix)
        return self.bn_fwd_args(st, prefix, moving=False), 0

    def conv(self, xin, wname, bname, dil, out, swish_stats, x_scale=None, border_bias=None, out_block=0, part=None, bnin=None):
        """dense conv; in training the epilogue also emits the following BN's statistics (returns their block count) into
        P.stats_part, or `part`.  bnin: the batch norm in front of this conv (the previous block's project BN, deferred: see
        _mbconv_tail_fwd) applied while the conv loads its rows -- xin is then that batch norm's OUTPUT buffer, written by the launch."""
        L, P, w = self.L, self.P, self.w
        am = L._amax_of.get(wname)
        if bnin is not None:
            return ops.conv2d_fwd_bnin(bnin["z"], P.stats_part3, bnin["nblk"], *self.bn_bwd_args(bnin["st"], bnin["prefix"]), xin, w[wname], out,
                                       moving=self.moving(bnin["prefix"]), img_scale=bnin["img_scale"], res=bnin["res"], stats_part=P.stats_part,
                                       stats_swish=swish_stats, wt=L.wt[wname], precision=L.matmul_precision, fp8_w_amax=am, out_block=out_block)[1]
        part = (P.stats_part if part is None else part) if self.training else None
        bias, swish_stats = (w[bname] if bname else None), bool(swish_stats and self.training)
        if L._x3_takes(wname, xin):   # (fp32x3: a long-K decoder conv on a map large enough to fill the chip)
            r = ops.conv2d_fwd_x3(xin, L.x3.image(wname, "fwd"), w[wname].shape[0], w[wname].shape[3], bias, dil, out=out, ws=self.ws,
                                  stats_part=part, stats_swish=swish_stats, border_bias=border_bias)
        else:
            r = L._conv_fwd(xin, w[wname], bias, dil, out=out, ws=self.ws, stats_part=part, stats_swish=swish_stats, wt=L.wt[wname],
                            x_scale=x_scale, border_bias=border_bias, fp8_w_amax=am, out_block=out_block)
        return r[1] if self.training else 0

    def dwconv(self, xin, wname, stride, out):
        """depthwise conv; in training the launch also leaves the following BN's stage-1 statistics in P.stats_part (returns their
        block count)."""
        if self.training:
            return ops.dwconv_fwd(xin, self.w[wname], stride, out=out, stats_part=self.P.stats_part)[1]
        ops.dwconv_fwd(xin, self.w[wname], stride, out=out)
        return 0

    def bn_b(self, xin, dy, st, prefix, dx, pre=False, post=False, img_scale=None, chan_scale=None, chan_add=None, dskip=None,
             dskip_accumulate=False, dxsum_part=None, stage1=None):
        ops.bn_bwd(xin, dy, *self.bn_bwd_args(st, prefix), pre, post, img_scale, chan_scale, chan_add, dx=dx, dgamma=self.g[prefix + "/gamma"],
                   dbeta=self.g[prefix + "/beta"], ws=self.ws, dskip=dskip, dskip_accumulate=dskip_accumulate, dxsum_part=dxsum_part, stage1=stage1)

    def wgrad_conv(self, xin, dz, kk, dil, key, x_scale=None):
        """filter gradient of a dense conv (slabs into P.fold_part[key]): deferred into the plan's batch, launched at the end of the
        pass, one launch per kernel instantiation.  (Round 4 ran the decoder's share on a side branch of the captured step with
        capped grids beside the encoder's backward chain: neutral to negative.  Round 5 ran it as a graph of its own on a stream
        masked to 64-96 CUs beside the chain on the other 160-192: the masks hold, the chain slows by what the move saves --
        profiles/r05_notes.md -- removed again.)"""
        P = self.P
        if not P.wbatch_ready:
            P.wbatch.add(xin, dz, kk, dil, P.fold_part[key], x_scale=x_scale)

    def conv_bwd_data(self, dz, wname, dil, cin, out, accumulate=False):
        """backward-data of a decoder 3x3 conv into its first `cin` input channels: fp32x3 where the forward conv took it."""
        L = self.L
        if L._x3_takes(wname, dz):
            ops.conv2d_bwd_data_x3(dz, L.x3.image(wname, "bwd"), 3, cin, dil, out=out, accumulate=accumulate, ws=self.ws)
        else:
            L._conv_bwd_data(dz, self.w[wname], dil, ci_begin=0, ci_count=cin, out=out, accumulate=accumulate, ws=self.ws)

    def noexpand_dw_bwd(self, B, tgt, tgt_has, dw_bwd_data):
        """Block without an expand conv: dw_bwd_data(out), its depthwise backward-data launch, into the block-input gradient tgt.  With
        the identity skip's share already there (EfficientNet-B3 stage-1 repeats) through B["da0"] and an accumulate."""
        if tgt_has:
            dw_bwd_data(B["da0"])
            ops.chan_affine(B["da0"], out=tgt, accumulate=True)
        else:
            dw_bwd_data(tgt)


class _Passes:
    X3_MIN_ROWS = 8192   # fp32x3 only on maps with at least this many pixels in the batch (32 row tiles of 256): below, the stream-K
                         # parts are a few chunks each and the native kernel wins (14x14 level: 31 against 20 us per launch)

    def _x3_takes(self, wname, xin) -> bool:
        return self.x3 is not None and self.x3.has(wname, "fwd") and xin.shape[0] * xin.shape[1] * xin.shape[2] >= self.X3_MIN_ROWS

    # ------------------------------------------------------------------------------------------- forward
    def _forward(self, P: _Plan, x, idx, training: bool, upsample: bool = True, stochastic: bool = True):
        """stochastic=False (predict): training mode means batch statistics only -- no drop-connect scale and no dropout mask is read,
        so the plan's mask buffers (never written outside a training step) stay out of the result."""
        a, S = self.arch, _Pass(self, P, training, stochastic)
        # (the weight shadows of the step and -- in a training step that draws its masks on the device -- the masks: ONE launch)
        ops.transpose_weights(self.arena.theta, self.theta_t, self.wt_desc, self.w_amax, tiles=self.wt_tiles, x3=self.x3, rng=self._rng_now)
        self._rng_now = None
        cur, nb_stem = self._stem_fwd(S, x, idx)
        pend = None   # the previous block's project batch norm, when this block's expand conv applies it on load (P.bn2_deferred)
        for bi, (b, B, nm) in enumerate(zip(a.executed(), P.blocks, self.n_blocks)):
            B["x_in"] = cur
            if training and B["small"]:
                cur, pend = self._mbconv_small_fwd(S, bi, b, B, nm, cur, pend)
            elif B["march"]:
                cur, pend = self._mbconv_march_fwd(S, bi, b, B, nm, cur, pend, nb_stem)
            else:
                cur, pend = self._mbconv_opbyop_fwd(S, bi, b, B, nm, cur, pend)
        if pend is not None:
            raise MliisError("internal: a deferred project batch norm was not consumed")
        ends = {r: P.blocks[bi]["out"] for r, bi in a.reductions.items() if bi < len(P.blocks)}
        dec = ends[4]
        if a.aspp:
            dec = self._aspp_forward(P, dec, S.stochastic)
        if a.skipdec is not None:
            dec = self._skipdec_fwd(S, dec, ends)
        for j in range(len(a.rsd)):
            dec = self._rsd_fwd(S, j, dec, ends)
        mask = P.drop_mask if (S.stochastic and P.drop_mask is not None) else None
        P.dec_in = dec
        ops.final_conv_fwd(dec, S.w[self.n_final[0]], S.w[self.n_final[1]], mask, out=P.small)
        H = a.image_size
        if not upsample:   # (the fused head launch reads the decoder-resolution logits: Learner._train_sequence)
            return None
        ops.resize_bilinear_fwd(P.small, (H, H), out=P.logits)
        return P.logits

    def _stem_fwd(self, S: _Pass, x, idx):
        """Stem conv -> BN -> swish.  Returns (activation, 0), or (None, blocks of stage-1 statistics in P.stats_part) when block 0's
        depthwise launch takes the stem's BN + swish (P.fuse_stem: _Plan)."""
        P, w = S.P, S.w
        # training: the stem conv's launch also leaves the stage-1 statistics of its batch norm (row-strip kernel; -1: the rows are too
        # wide for it -- the plain kernel ran and the consumer takes the statistics launch)
        nb = 0
        if S.training:
            nb = max(0, ops.stem_conv_fwd(x, w[self.n_stem[0]], idx, out=P.z_stem, stats_part=P.stats_part)[1])
        else:
            ops.stem_conv_fwd(x, w[self.n_stem[0]], idx, out=P.z_stem)
        if P.fuse_stem:
            return None, nb
        return S.bn(P.z_stem, P.st_stem, self.n_stem[1], P.a_stem, post=True, nblk=nb), 0

    def _mbconv_small_fwd(self, S: _Pass, bi, b, B, nm, x, bnin):
        """Small-map fused block (training): expand GEMM (+ stage-1 statistics) -> ONE launch: bn0 fold + apply + swish, depthwise, bn1
        statistics + apply + swish, squeeze-excite means, both moving averages -> SE MLP -> project GEMM."""
        P, w = S.P, S.w
        z0 = B["z0b"] if B["blk"] else B["z0"]     # (blk: the expand conv writes the group-blocked layout itself)
        nb = S.conv(x, nm["w_exp"], None, 1, z0, False, out_block=B["blk"], bnin=bnin)
        if nb == 0:
            if B["blk"]:
                raise MliisError("internal: the streamed expand conv of block {} left no statistics".format(b.idx))
            nb = ops.bn_stats_partial(z0, False, P.stats_part)
        ops.mbconv_dw_fwd_small(z0, P.stats_part, nb, S.bn_fwd_args(B["st0"], nm["bn0"]), w[nm["w_dw"]], S.bn_fwd_args(B["st1"], nm["bn1"]),
                                B["z1"], B["a1"], B["s"], z0_blocked=B["z0b"], z1_blocked=True)   # (the backward's re-reads: contiguous)
        return self._mbconv_tail_fwd(S, bi, b, B, nm)

    def _mbconv_march_fwd(self, S: _Pass, bi, b, B, nm, x, bnin, nb_stem):
        """Row-marching block: expand GEMM (+ stage-1 statistics) -> ONE launch: bn0 fold + apply + swish while the rows are staged,
        depthwise conv, bn1 stage-1 statistics (P.stats_part2) -> bn1 + swish + pooling -> SE MLP -> project GEMM."""
        P, w = S.P, S.w
        if b.expand != 1:
            nb = S.conv(x, nm["w_exp"], None, 1, B["z0"], False, bnin=bnin)
            bn0, nb = S.bn_in(B["z0"], B["st0"], nm["bn0"], nb)
            zin = B["z0"]
        elif bi == 0 and P.fuse_stem:
            bn0, nb = S.bn_in(P.z_stem, P.st_stem, self.n_stem[1], nb_stem)
            zin = P.z_stem
        else:
            bn0, nb, zin = None, 0, x
        if S.training:
            nb = ops.dwconv_bn_fwd(zin, w[nm["w_dw"]], b.stride, bn=bn0, part=P.stats_part, nblk=nb, out=B["z1"], stats_part=P.stats_part2)[1]
        else:
            ops.dwconv_bn_fwd(zin, w[nm["w_dw"]], b.stride, bn=bn0, out=B["z1"])
            nb = 0
        return self._mbconv_bn1_fwd(S, bi, b, B, nm, nb, P.stats_part2)

    def _mbconv_opbyop_fwd(self, S: _Pass, bi, b, B, nm, x, bnin):
        """Op-by-op block: expand GEMM -> bn0 + swish -> depthwise conv -> bn1 + swish + pooling -> SE MLP -> project GEMM."""
        if b.expand != 1:
            nb = S.conv(x, nm["w_exp"], None, 1, B["z0"], False, bnin=bnin)
            x = S.bn(B["z0"], B["st0"], nm["bn0"], B["a0"], post=True, nblk=nb)
        nb = S.dwconv(x, nm["w_dw"], b.stride, B["z1"])
        return self._mbconv_bn1_fwd(S, bi, b, B, nm, nb, S.P.stats_part)

    def _mbconv_bn1_fwd(self, S: _Pass, bi, b, B, nm, nb, st_part):
        """bn1 + swish on the depthwise output (its nb blocks of stage-1 statistics in st_part) with the squeeze-excite pooling, then
        the block's tail."""
        P = S.P
        if S.training:   # bn1's apply pass also pools its output per image (partial sums); the SE kernel folds them
            chunks = S.bn(B["z1"], B["st1"], nm["bn1"], B["a1"], post=True, nblk=nb, pool_part=P.pool_part, part=st_part)[1]
            return self._mbconv_tail_fwd(S, bi, b, B, nm, pool_chunks=chunks)
        S.bn(B["z1"], B["st1"], nm["bn1"], B["a1"], post=True, nblk=nb)
        ops.colsum(B["a1"], None, nseg=P.N, scale=1.0 / (b.h_out * b.h_out), out=B["s"], ws=S.ws)
        return self._mbconv_tail_fwd(S, bi, b, B, nm)

    def _mbconv_tail_fwd(self, S: _Pass, bi, b, B, nm, pool_chunks=None):
        """The tail of every MBConv block: SE MLP on the pooled means B["s"] (pool_chunks: on the partial sums in P.pool_part) -> gated
        project GEMM -> the block's project batch norm (+ drop-connect scale, + identity skip): a launch of its own, or -- training, the
        next block's expand conv on the streamed plan -- handed to that conv, which forms the block output while it loads its rows and
        writes it to B["out"] (ops.conv2d_fwd_bnin: one launch and one pass over z2 less per block).  Returns (output, hand-over | None)."""
        P = S.P
        se = [S.w[k] for k in nm["se"]]
        if pool_chunks is None:
            ops.se_mlp_fwd(B["s"], *se, B["hpre"], B["gate"])
        else:
            ops.se_mlp_fwd(P.pool_part, *se, B["hpre"], B["gate"], chunks=pool_chunks, scale=1.0 / (b.h_out * b.h_out), s_out=B["s"])
        defer = S.training and P.bn2_deferred[bi]
        # squeeze-excite gate applied inside the project GEMM's A loader (the gated tensor is never written)
        nb = S.conv(B["a1"], nm["w_proj"], None, 1, B["z2"], False, x_scale=B["gate"], part=P.stats_part3 if defer else None)
        use_dc = B["use_dc"] = S.stochastic and self.drop_connect and b.skip and b.drop_rate > 0
        img_scale, res = (B["dc"] if use_dc else None), (B["x_in"] if b.skip else None)
        if defer:
            if nb == 0:
                nb = ops.bn_stats_partial(B["z2"], False, P.stats_part3)
            return B["out"], dict(z=B["z2"], nblk=nb, st=B["st2"], prefix=nm["bn2"], img_scale=img_scale, res=res)
        return S.bn(B["z2"], B["st2"], nm["bn2"], B["out"], img_scale=img_scale, res=res, nblk=nb), None

    def _skipdec_fwd(self, S: _Pass, dec, ends):
        """The --skip_decoding decoder, efficientlab.py:133-149: [resize(embedded, input // 4) | swish(BN(conv1x1(reduction_2)))] -> two
        sep_convs (dw 3x3 -> BN -> swish -> 1x1 -> BN -> swish).  Every BN here is built with training=True in the reference."""
        sd, T = self.arch.skipdec, S.P.skipdec
        (k0, n0), seps = self.n_skipdec
        cur = T["cat"]
        ops.resize_bilinear_fwd(dec, (sd.h, sd.h), out=cur[..., :sd.c_in])
        nb = S.conv(ends[2], k0, None, 1, T["z0"], False)
        S.bn(T["z0"], T["st0"], n0, cur[..., sd.c_in:], post=True, fused=True, nblk=nb, always_batch=True)
        for Q, (dwn, dbn, pwn, pbn) in zip(T["sep"], seps):
            Q["x_in"] = cur
            nb = S.dwconv(cur, dwn, 1, Q["zd"])
            S.bn(Q["zd"], Q["std"], dbn, Q["ad"], post=True, fused=True, nblk=nb, always_batch=True)
            nb = S.conv(Q["ad"], pwn, None, 1, Q["zp"], False)
            cur = S.bn(Q["zp"], Q["stp"], pbn, Q["out"], post=True, fused=True, nblk=nb, always_batch=True)
        return cur

    def _rsd_fwd(self, S: _Pass, j, dec, ends):
        """Residual skip decoder module j on the deep map `dec` and its skip endpoint."""
        P, w, ws = S.P, S.w, S.ws
        m, D, nm = self.arch.rsd[j], P.rsd[j], self.n_rsd[j]
        skip = ends[m.scope_index + 1]
        cat = D["cat"]
        up = cat[..., :m.c_deep]
        # the concat of the (resized) deep map and the skip feature, and the pooled branch's per-image sums of it: one launch
        pool_chunks = 0
        if m.c_deep % 4 == 0 and (m.c_cat - m.c_deep) % 4 == 0 and m.h > 1:
            pool_chunks = ops.rsd_concat_pool(dec, skip, cat, D["pool_part"])
        else:
            if m.h_in == m.h:
                ops.chan_affine(dec, out=up)
            else:
                ops.resize_bilinear_fwd(dec, (m.h, m.h), out=up)
            ops.chan_affine(skip, out=cat[..., m.c_deep:])
        res_up = up
        if m.upsample_conv:   # the residual operand through its own conv -> swish -> BN branch; the concat keeps the resized map
            ku, bu, nu = self.n_rsd_up[j]
            nb = S.conv(up, ku, bu, 1, D["zu"], True)
            res_up = S.bn(D["zu"], D["stu"], nu, D["up2"], pre=True, fused=True, nblk=nb)
        pyr = D["pyr"]
        (k0, b0, n0), (k1, b1, n1), (kf, bf, nf) = nm
        if S.training:
            # the 1x1 and the 3x3-dilated branch are independent: both GEMMs first (statistics in two buffers), then ONE launch for
            # the two conv -> swish -> BN tails
            nb0 = S.conv(cat, k0, b0, 1, D["z0"], True)
            nb1 = S.conv(cat, k1, b1, 2, D["z1"], True, part=P.stats_part2)
            ops.bn_apply_fused_pair([(D["z" + i], pt, nb_, *S.bn_bwd_args(D["st" + i], nn), S.moving(nn), out_)
                                     for i, pt, nb_, nn, out_ in (("0", P.stats_part, nb0, n0, pyr[..., :m.c_out]),
                                                                  ("1", P.stats_part2, nb1, n1, pyr[..., m.c_out:2 * m.c_out]))],
                                    pre_swish=True, unbiased_moving_var=True)
        else:
            nb = S.conv(cat, k0, b0, 1, D["z0"], True)
            S.bn(D["z0"], D["st0"], n0, pyr[..., :m.c_out], pre=True, fused=True, nblk=nb)
            nb = S.conv(cat, k1, b1, 2, D["z1"], True)
            S.bn(D["z1"], D["st1"], n1, pyr[..., m.c_out:2 * m.c_out], pre=True, fused=True, nblk=nb)
        # pooled branch: per-image mean of `cat`, folded into the fuse conv as a border-class bias (rsd.hip)
        if pool_chunks:
            ops.rsd_pool_fwd(D["pool_part"], w[kf], 2 * m.c_out, out=D["bbias"], chunks=pool_chunks, scale=1.0 / (m.h * m.h), pool_out=D["pool"])
        else:
            ops.colsum(cat, None, nseg=P.N, scale=1.0 / (m.h * m.h), out=D["pool"], ws=ws)
            ops.rsd_pool_fwd(D["pool"], w[kf], 2 * m.c_out, out=D["bbias"])
        nb = S.conv(pyr, kf, bf, 1, D["zf"], True, border_bias=D["bbias"])
        return S.bn(D["zf"], D["stf"], nf, D["out"], pre=True, res=res_up, fused=True, nblk=nb)

    # ------------------------------------------------------------------------------------------- ASPP (--spatial_pyramid_pooling)
    def _aspp_forward(self, P: _Plan, x, dropout: bool):
        """models/efficientlab.py:248-289 on the encoder output x [N,h,h,Cin]: 1x1 / 3x3-dilation-6 / image-pooling branches written
        straight into channel slices of the concat buffer ([pooled | 3x3 | 1x1], the reference's order), then 1x1 conv + swish +
        dropout.  The dense convs are the MFMA implicit GEMM, the activations mliis_swish_mask_*."""
        a, w, ws, T, N = self.arch, self.arena.w, self.ws, P.aspp, P.N
        d, hw = a.aspp_dimension, a.aspp_h * a.aspp_h
        (k0, c0), (k1, c1), (k2, c2), (ko, co) = self.n_aspp
        m = T["masks"] if dropout else [None] * 4
        cat = T["cat"]
        self._conv_fwd(x, w[k0], w[c0], 1, out=T["z0"], ws=ws, wt=self.wt[k0], fp8_w_amax=self._amax_of.get(k0))
        ops.swish_mask_fwd(T["z0"], m[0], out=cat[..., 2 * d:])
        self._conv_fwd(x, w[k1], w[c1], spec.ASPP_DILATION, out=T["z1"], ws=ws, wt=self.wt[k1])
        ops.swish_mask_fwd(T["z1"], m[1], out=cat[..., d:2 * d])
        ops.colsum(x, None, nseg=N, scale=1.0 / hw, out=T["pool"], ws=ws)
        self._conv_fwd(T["pool"].view(N, 1, 1, -1), w[k2], w[c2], 1, out=T["z2"].view(N, 1, 1, d), ws=ws, wt=self.wt[k2],
                       fp8_w_amax=self._amax_of.get(k2))
        ops.swish_mask_fwd(T["z2"], m[2], out=T["b2"], pre_mask=True)
        ops.chan_affine(None, A=T["b2"], out=cat[..., :d])      # bilinear resize of the 1x1 pooled map = broadcast
        self._conv_fwd(cat, w[ko], w[co], 1, out=T["zo"], ws=ws, wt=self.wt[ko], fp8_w_amax=self._amax_of.get(ko))
        ops.swish_mask_fwd(T["zo"], m[3], out=T["out"])
        T["trained"] = dropout
        return T["out"]

    def _aspp_backward(self, P: _Plan, x, dx, dx_has: bool):
        """Gradients of the ASPP parameters (straight into the gradient arena) and of its input (accumulated into dx when dx_has)."""
        a, A, ws, T, N = self.arch, self.arena, self.ws, P.aspp, P.N
        w, g = A.w, A.g
        d, hw = a.aspp_dimension, a.aspp_h * a.aspp_h
        (k0, c0), (k1, c1), (k2, c2), (ko, co) = self.n_aspp
        m = T["masks"]
        cat, dcat = T["cat"], T["dcat"]
        dzo = ops.swish_mask_bwd(T["dout"], T["zo"], m[3], out=T["dzo"])
        self._conv_bwd_filter(cat, dzo, 1, 1, out=g[ko], ws=ws)
        ops.colsum(dzo, out=g[co], ws=ws)
        self._conv_bwd_data(dzo, w[ko], 1, out=dcat, ws=ws)
        # 1x1 branch (the pre-activation gradient overwrites its slice of dcat)
        d0 = ops.swish_mask_bwd(dcat[..., 2 * d:], T["z0"], m[0], out=dcat[..., 2 * d:])
        self._conv_bwd_filter(x, d0, 1, 1, out=g[k0], ws=ws)
        ops.colsum(d0, out=g[c0], ws=ws)
        self._conv_bwd_data(d0, w[k0], 1, out=dx, accumulate=dx_has, ws=ws)
        # 3x3 dilation-6 branch
        d1 = ops.swish_mask_bwd(dcat[..., d:2 * d], T["z1"], m[1], out=dcat[..., d:2 * d])
        self._conv_bwd_filter(x, d1, 3, spec.ASPP_DILATION, out=g[k1], ws=ws)
        ops.colsum(d1, out=g[c1], ws=ws)
        self._conv_bwd_data(d1, w[k1], spec.ASPP_DILATION, out=dx, accumulate=True, ws=ws)
        # image-pooling branch: per-image sums of the broadcast slice -> [N, d] chain -> mean's gradient on every pixel
        ops.colsum(dcat[..., :d], None, nseg=N, out=T["db2"], ws=ws)
        d2 = ops.swish_mask_bwd(T["db2"], T["z2"], m[2], out=T["db2"], pre_mask=True)
        pool4, d24 = T["pool"].view(N, 1, 1, -1), d2.view(N, 1, 1, d)
        self._conv_bwd_filter(pool4, d24, 1, 1, out=g[k2], ws=ws)
        ops.colsum(d2, out=g[c2], ws=ws)
        self._conv_bwd_data(d24, w[k2], 1, out=T["dpool"].view(N, 1, 1, -1), ws=ws)
        ops.axpby(0.0, None, 1.0 / hw, T["dpool"])                       # d(mean)/dx = 1 / (h*w) on every pixel
        ops.chan_affine(None, A=T["dpool"], out=dx, accumulate=True)

    # ------------------------------------------------------------------------------------------- backward
    def _backward(self, P: _Plan, x, idx, head_fused: bool = False):
        a, S = self.arch, _Pass(self, P, True)
        w, g = S.w, S.g
        if not head_fused:   # (ops.head_ce_fused left the gradient on the decoder's map already)
            ops.resize_bilinear_bwd(P.dlogits, (a.h_dec, a.h_dec), out=P.dsmall)
        mask = P.drop_mask
        ops.final_conv_bwd_filter(P.dec_in, P.dsmall, mask, dw=g[self.n_final[0]], db=g[self.n_final[1]], ws=S.ws)
        has_grad = [False] * len(P.blocks)   # has_grad[i]: block i's dout already holds a contribution (the next one accumulates)
        dtop, _ = self._deep_grad_target(P, has_grad, len(a.rsd))
        ops.final_conv_bwd_data(P.dsmall, w[self.n_final[0]], a.c_final, mask, out=dtop, fin=P.head_fin if head_fused else None)
        if not P.wbatch_ready:   # (a first backward pass that raised half-way must not leave half a table behind)
            P.wbatch = ops.FilterBatch(self.device)
        for j in range(len(a.rsd) - 1, -1, -1):
            self._rsd_bwd(S, j, has_grad)
        if a.skipdec is not None:
            self._skipdec_bwd(S, has_grad)
        if a.aspp:
            bi = a.reductions[4]
            self._aspp_backward(P, P.blocks[bi]["out"], P.blocks[bi]["dout"], has_grad[bi])
            has_grad[bi] = True
        # stage1: stage 1 of the batch-norm backward the NEXT stage down starts with (block bi - 1's project BN; below block 0 the
        # stem's BN), when the launch that completed its input gradient also produced it
        stage1 = None
        ex = a.executed()
        for bi in range(len(P.blocks) - 1, -1, -1):
            b, B, nm = ex[bi], P.blocks[bi], self.n_blocks[bi]
            if not has_grad[bi]:
                raise MliisError("internal: block {} has no upstream gradient".format(bi))
            # gradient for the block input
            tgt = P.blocks[bi - 1]["dout"] if bi > 0 else P.dstem
            tgt_has = has_grad[bi - 1] if bi > 0 else False
            if B["small"]:
                stage1 = self._mbconv_small_bwd(S, bi, b, B, nm, tgt, tgt_has, stage1)
            elif B["march"]:
                stage1 = self._mbconv_march_bwd(S, bi, b, B, nm, tgt, tgt_has, stage1)
            else:
                stage1 = self._mbconv_opbyop_bwd(S, bi, b, B, nm, tgt, tgt_has, stage1)
            if bi > 0:
                has_grad[bi - 1] = True
        self._stem_bwd(S, x, idx, stage1)
        P.wbatch_ready = True
        P.wbatch.launch("fp32x3" if self.x3 is not None else self.matmul_precision)
        # all slabs written -> one batched fold into the gradient arena; the squeeze-excite weight gradients of every block ride in it
        ops.fold_batched(P.fold_buf, self.arena.grad, P.fold_desc, P.fold_tiles, se_desc=P.se_desc, se_tiles=P.se_tiles)

    def _deep_grad_target(self, P: _Plan, has_grad, j):
        """(buffer, accumulate) for the gradient w.r.t. the deep input of decoder stage j (an RSD module; -1: the --skip_decoding
        decoder; len(rsd): the final conv): the `dout` of the stage in front of it, or of the encoder's last block, marked in has_grad."""
        a = self.arch
        if j > 0:
            return P.rsd[j - 1]["dout"], False
        if j == 0 and a.skipdec is not None:
            return P.skipdec["dout"], False
        if a.aspp:
            return P.aspp["dout"], False
        bi = a.reductions[4]
        tgt_has, has_grad[bi] = has_grad[bi], True
        return P.blocks[bi]["dout"], tgt_has

    def _rsd_bwd(self, S: _Pass, j, has_grad):
        """Residual skip decoder module j: from D["dout"] into the gradients of its skip endpoint and of its deep input."""
        a, P, w, g, ws = self.arch, S.P, S.w, S.g, S.ws
        m, D, nm = a.rsd[j], P.rsd[j], self.n_rsd[j]
        (k0, b0, n0), (k1, b1, n1), (kf, bf, nf) = nm
        co = m.c_out
        dO, cat, pyr, dpyr, dcat = D["dout"], D["cat"], D["pyr"], D["dpyr"], D["dcat"]
        S.bn_b(D["zf"], dO, D["stf"], nf, D["dzf"], pre=True)
        ops.rsd_pool_bwd(D["dzf"], D["tot"], D["pool"], w[kf], 2 * co, dw=g[kf], dbias=g[bf], dpool=D["dpool"], ws=ws)
        S.wgrad_conv(pyr, D["dzf"], 3, 1, kf)   # rows of the 2*co convolved channels
        S.conv_bwd_data(D["dzf"], kf, 1, 2 * co, dpyr)
        d0, d1 = dpyr[..., :co], dpyr[..., co:2 * co]
        # both branches' batch norms: one reduce launch + one apply launch (+ conv-bias gradient slabs for the batched fold)
        ops.bn_bwd_pair([(D["z" + i], d_, *S.bn_bwd_args(D["st" + i], nn), d_, g[nn + "/gamma"], g[nn + "/beta"], P.fold_part[bb])
                         for i, d_, nn, bb in (("0", d0, n0, b0), ("1", d1, n1, b1))], pre_swish=True, ws=ws)
        tail = P.filter_tail[j]
        cmain = cat[..., :m.c_cat - tail] if tail else cat

        def wgrad(dz, kname, kk, dil, cmain=cmain, ctail=cat[..., m.c_cat - tail:] if tail else None):
            S.wgrad_conv(cmain, dz, kk, dil, kname)
            if ctail is not None:   # the <= 16-channel sliver of the concat (see _Plan)
                S.wgrad_conv(ctail, dz, kk, dil, kname + "#tail")
        wgrad(d0, k0, 1, 1)
        self._conv_bwd_data(d0, w[k0], 1, out=dcat, ws=ws)
        wgrad(d1, k1, 3, 2)
        S.conv_bwd_data(d1, k1, 2, m.c_cat, dcat, accumulate=True)
        # gradient of the concat = dcat + dpool / (H*W) on every pixel (the pooled branch); its deep half joins the residual
        # gradient, its skip half goes to the endpoint's gradient: one pass (mliis_chan_split)
        bi_skip = a.reductions[m.scope_index + 1]
        if m.upsample_conv:
            # the residual operand came through its own conv -> swish -> BN branch (efficientlab.py:213-215): dO is its gradient;
            # back through that branch to the resized deep map, where the concat's share joins
            ku, bu, nu = self.n_rsd_up[j]
            S.bn_b(D["zu"], dO, D["stu"], nu, D["dzu"], pre=True, dxsum_part=P.fold_part[bu])
            S.wgrad_conv(cat[..., :m.c_deep], D["dzu"], 1, 1, ku)
            self._conv_bwd_data(D["dzu"], w[ku], 1, out=D["dup"], ws=ws)
            dU = D["dup"]
        else:
            dU = dO      # dU = dO + dcat[:, :c_deep] (residual)
        ops.chan_split(dcat, m.c_deep, dU, True, P.blocks[bi_skip]["dout"], has_grad[bi_skip], A=D["dpool"])
        has_grad[bi_skip] = True
        # gradient w.r.t. the deep input (for RSD(4) without a decoder in front it is the same endpoint the skip half just went to)
        tgt, tgt_has = self._deep_grad_target(P, has_grad, j)
        if m.h_in == m.h:
            ops.chan_affine(dU, out=tgt, accumulate=tgt_has)
        else:
            ops.resize_bilinear_bwd(dU, (m.h_in, m.h_in), out=tgt, accumulate=tgt_has)

    def _skipdec_bwd(self, S: _Pass, has_grad):
        """--skip_decoding decoder backward: the two sep_convs in reverse, then the concat's two halves -- the projected reduction_2
        endpoint (conv1x1 -> BN -> swish) and the resized embedded image."""
        a, P, w, ws = self.arch, S.P, S.w, S.ws
        sd, T = a.skipdec, P.skipdec
        (k0, n0), seps = self.n_skipdec
        d = T["dout"]     # from the first RSD module (or, without RSD modules, the final conv's input gradient)
        for Q, (dwn, dbn, pwn, pbn) in zip(reversed(T["sep"]), reversed(seps)):
            S.bn_b(Q["zp"], d, Q["stp"], pbn, d, post=True)
            S.wgrad_conv(Q["ad"], d, 1, 1, pwn)
            self._conv_bwd_data(d, w[pwn], 1, out=Q["dad"], ws=ws)
            S.bn_b(Q["zd"], Q["dad"], Q["std"], dbn, Q["dad"], post=True)
            ops.dwconv_bwd_filter(Q["x_in"], Q["dad"], 3, 1, partial=P.fold_part[dwn])
            ops.dwconv_bwd_data(Q["dad"], w[dwn], 1, (sd.h, sd.h), out=Q["din"])
            d = Q["din"]                              # (after the loop: the concat's gradient [N, h, h, c_in + c_skip])
        bi2 = a.reductions[2]
        S.bn_b(T["z0"], d[..., sd.c_in:], T["st0"], n0, T["dz0"], post=True)
        S.wgrad_conv(P.blocks[bi2]["out"], T["dz0"], 1, 1, k0)
        self._conv_bwd_data(T["dz0"], w[k0], 1, out=P.blocks[bi2]["dout"], accumulate=has_grad[bi2], ws=ws)
        has_grad[bi2] = True
        tgt, tgt_has = self._deep_grad_target(P, has_grad, -1)
        ops.resize_bilinear_bwd(d[..., :sd.c_in], (sd.h_in, sd.h_in), out=tgt, accumulate=tgt_has)

    def _mbconv_project_bwd(self, S: _Pass, b, B, nm, tgt, tgt_has, stage1, out_block=0, bn1_sums=True):
        """The head of every MBConv backward, from the block's output gradient to B["da2"], the gradient of the gated depthwise activation:
        project BN (+ the identity skip's share of the block-input gradient into tgt), project conv, squeeze-excite.  out_block: da2 in
        the small-map kernels' group-blocked layout; bn1_sums: the squeeze-excite pass may also produce stage 1 of bn1's backward.
        Returns (tgt_has, that stage 1 or None)."""
        P, w, ws, N = S.P, S.w, S.ws, S.P.N
        dout, da2, hw = B["dout"], B["da2"], b.h_out * b.h_out
        # identity-skip part of the block-input gradient: written by the same pass that turns dout into the bn2 input gradient
        S.bn_b(B["z2"], dout, B["st2"], nm["bn2"], dout, img_scale=B["dc"] if B["use_dc"] else None,
               dskip=tgt if b.skip else None, dskip_accumulate=tgt_has, stage1=stage1)
        S.wgrad_conv(B["a1"], dout, 1, 1, nm["w_proj"], x_scale=B["gate"])
        se = nm["se"]
        groups = 0
        if 16 <= hw <= 256:
            # small maps: the project backward-data launch also leaves the gate gradient's per-row-group partial sums of da2 * a1
            # and the SE kernel folds them -- no pass over the two tensors (mliis_conv2d_bwd_data_gate)
            _, groups = self._conv_bwd_data(dout, w[nm["w_proj"]], 1, out=da2, ws=ws, gate=B["a1"], part=P.gate_part, out_block=out_block)
        else:
            self._conv_bwd_data(dout, w[nm["w_proj"]], 1, out=da2, ws=ws)
        se_outs = dict(dpre1=B["dpre1"], dpre2=B["dpre2"], chan_add=B["chan_add"])
        if not groups and bn1_sums:
            # ONE pass over (da2, z1): the gate's gradient and everything bn1's backward needs from the two tensors; the SE kernel
            # folds it and emits bn1's stage-1 sums per image -- no column-sum launch, no reduce pass of the batch norm
            nbs = ops.se_bn_bwd_sums(B["z1"], da2, *S.bn_bwd_args(B["st1"], nm["bn1"]), P.sums_part)
            ops.se_mlp_bwd_bn(P.sums_part, nbs, B["gate"], B["hpre"], w[se[0]], w[se[2]], hw, se_outs, P.stage1_se, w1t=self.wt[se[0]])
            return tgt_has or b.skip, (P.stage1_se, N)
        if not groups:
            if out_block:   # (da2 is group-blocked here, a1 is not: their product needs the launch's own partial sums)
                raise MliisError("internal: the project backward-data launch of block {} left no gate-gradient partials for its "
                                 "group-blocked output".format(b.idx))
            ops.colsum(da2, B["a1"], nseg=N, out=B["dgate"], ws=ws)
        # (the SE weight gradients of all blocks are computed by one batched launch after the loop: P.se_desc)
        ops.se_mlp_bwd(P.gate_part if groups else B["dgate"], B["gate"], B["s"], B["hpre"], w[se[0]], w[se[2]], hw, se_outs,
                       dgate_groups=groups, w1t=self.wt[se[0]])
        return tgt_has or b.skip, None

    def _mbconv_expand_bwd(self, S: _Pass, bi, B, nm, da0, tgt, tgt_has):
        """The tail of every MBConv backward with an expand conv: its filter gradient, and its backward-data into the gradient of
        block bi - 1's output -- the last contribution to it, so the launch can also emit stage 1 of that block's project-BN backward
        (mliis_conv2d_bwd_data_bn; small maps only), which is returned."""
        P, w = S.P, S.w
        S.wgrad_conv(B["x_in"], da0, 1, 1, nm["w_exp"])
        if bi == 0:
            self._conv_bwd_data(da0, w[nm["w_exp"]], 1, out=tgt, accumulate=tgt_has, ws=S.ws)
            return None
        Bp = P.blocks[bi - 1]
        _, nb = self._conv_bwd_data(da0, w[nm["w_exp"]], 1, out=tgt, accumulate=tgt_has, ws=S.ws,
                                    bn=(Bp["z2"], Bp["st2"][0], Bp["st2"][1], Bp["dc"] if Bp["use_dc"] else None), part=P.stats_part)
        return (P.stats_part, nb) if nb else None

    def _mbconv_small_bwd(self, S: _Pass, bi, b, B, nm, tgt, tgt_has, stage1):
        """Small-map fused block: project + squeeze-excite, then bn1 backward, depthwise filter gradient + backward-data, bn0 backward
        as one launch, then the expand conv."""
        w, g, p0, p1, da0 = S.w, S.g, nm["bn0"], nm["bn1"], B["da0"]
        tgt_has, _ = self._mbconv_project_bwd(S, b, B, nm, tgt, tgt_has, stage1, out_block=B["blk"], bn1_sums=False)
        ops.mbconv_dw_bwd_small(B["da2"], B["gate"], B["chan_add"], B["z1"], S.bn_bwd_args(B["st1"], p1), w[nm["w_dw"]], B["z0"],
                                S.bn_bwd_args(B["st0"], p0), g[p1 + "/gamma"], g[p1 + "/beta"], g[nm["w_dw"]], g[p0 + "/gamma"], g[p0 + "/beta"],
                                da0, z0_blocked=B["z0b"], z1_blocked=True, da2_blocked=bool(B["blk"]))
        return self._mbconv_expand_bwd(S, bi, B, nm, da0, tgt, tgt_has)

    def _mbconv_march_bwd(self, S: _Pass, bi, b, B, nm, tgt, tgt_has, stage1):
        """Row-marching block: project + squeeze-excite, then the depthwise half in one pass -- bn1's backward apply inside the launch
        (fuse_bn1) or as a launch of its own in front -- then bn0's backward and the expand conv.  Block 0 under P.fuse_stem: the stem's
        BN stands for bn0, tgt = P.dstem is the gradient w.r.t. the activated stem output, and stage 1 of that BN's backward is returned."""
        P, w, g, da2 = S.P, S.w, S.g, B["da2"]
        tgt_has, bn1_stage1 = self._mbconv_project_bwd(S, b, B, nm, tgt, tgt_has, stage1)
        wdw, slabs = w[nm["w_dw"]], P.fold_part[nm["w_dw"]]
        if b.expand != 1:
            zin, st0, p0, dxo = B["z0"], B["st0"], nm["bn0"], B["da0"]
        elif bi == 0 and P.fuse_stem:
            zin, st0, p0, dxo = P.z_stem, P.st_stem, self.n_stem[1], tgt
        else:
            zin = None
        # bn1's backward apply inside the depthwise backward launch (its operands are staged there anyway; dz1 is never written)
        # (not the 5x5 stride-1 layer: that instantiation spills, measured without gain -- profiles/r03_notes.md)
        fuse_bn1 = bn1_stage1 is not None and not (b.k == 5 and b.stride == 1) and zin is not None
        if not fuse_bn1:
            S.bn_b(B["z1"], da2, B["st1"], nm["bn1"], da2, post=True, chan_scale=B["gate"], chan_add=B["chan_add"], stage1=bn1_stage1)
        if zin is None:
            S.noexpand_dw_bwd(B, tgt, tgt_has, lambda out: ops.dwconv_bn_bwd(da2, B["x_in"], wdw, b.stride, out=out, dw_part=slabs))
            return None
        if fuse_bn1:
            p1, ce, N = nm["bn1"], b.cexp, P.N
            nb1 = ops.mbconv_dw_bwd_march(da2, B["z1"], S.bn_bwd_args(B["st1"], p1), B["gate"], B["chan_add"],
                                          P.stage1_se[:2 * N * ce].view(N, 2, ce), g[p1 + "/gamma"], g[p1 + "/beta"], zin,
                                          S.bn_bwd_args(st0, p0), wdw, b.stride, dxo, slabs, P.stats_part2)
        else:
            # ONE pass over (dz1, z0): depthwise backward-data, filter-gradient slabs and stage 1 of bn0's backward
            _, _, nb1 = ops.dwconv_bn_bwd(da2, zin, wdw, b.stride, bn=S.bn_bwd_args(st0, p0), out=dxo, dw_part=slabs, bn_part=P.stats_part2)
        if b.expand == 1:
            return P.stats_part2, nb1
        S.bn_b(B["z0"], dxo, st0, p0, dxo, post=True, stage1=(P.stats_part2, nb1))
        return self._mbconv_expand_bwd(S, bi, B, nm, dxo, tgt, tgt_has)

    def _mbconv_opbyop_bwd(self, S: _Pass, bi, b, B, nm, tgt, tgt_has, stage1):
        """Op-by-op block: project + squeeze-excite, bn1 backward, depthwise filter gradient and backward-data, bn0 backward, expand."""
        P, w, da2 = S.P, S.w, B["da2"]
        tgt_has, bn1_stage1 = self._mbconv_project_bwd(S, b, B, nm, tgt, tgt_has, stage1)
        S.bn_b(B["z1"], da2, B["st1"], nm["bn1"], da2, post=True, chan_scale=B["gate"], chan_add=B["chan_add"], stage1=bn1_stage1)
        ops.dwconv_bwd_filter(B["a0"] if b.expand != 1 else B["x_in"], da2, b.k, b.stride, partial=P.fold_part[nm["w_dw"]])
        if b.expand == 1:
            S.noexpand_dw_bwd(B, tgt, tgt_has, lambda out: ops.dwconv_bwd_data(da2, w[nm["w_dw"]], b.stride, (b.h_in, b.h_in), out=out))
            return None
        da0, st0 = B["da0"], B["st0"]
        # the depthwise backward-data launch also emits stage 1 of bn0's backward (sums over (z0, da0)): no reduce pass
        _, nb1 = ops.dwconv_bwd_data(da2, w[nm["w_dw"]], b.stride, (b.h_in, b.h_in), out=da0, part=P.stats_part,
                                     bn=(B["z0"],) + S.bn_bwd_args(st0, nm["bn0"]))
        S.bn_b(B["z0"], da0, st0, nm["bn0"], da0, post=True, stage1=(P.stats_part, nb1) if nb1 else None)
        return self._mbconv_expand_bwd(S, bi, B, nm, da0, tgt, tgt_has)

    def _stem_bwd(self, S: _Pass, x, idx, stage1):
        P = S.P
        S.bn_b(P.z_stem, P.dstem, P.st_stem, self.n_stem[1], P.dstem, post=True, stage1=stage1)
        ops.stem_conv_bwd_filter(x, P.dstem, idx, partial=P.fold_part[self.n_stem[0]])
