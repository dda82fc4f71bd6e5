"""The inner step on poisoned memory: a Learner whose plan buffers, workspaces and trainable gradient regions start as NaN (with guard
bands behind every buffer: tests/memcheck.py) must be BIT-identical to a Learner built on clean memory -- loss, every gradient, the
parameters, the batch-norm moving statistics and the logits of predict() in both modes.  Bit identity, not a tolerance: fmaxf and
compares swallow NaN, so a read-before-write can otherwise hide.  No oracle: cheap enough for full-size shapes."""
import numpy as np
import pytest
import torch

import memcheck as M

pytestmark = pytest.mark.gpu

# config name -> the entry points its steps must reach (besides what tests/test_memory_contract_gpu.py's cases reach)
REACHES = {
    "defaults": {"mliis_copy_words", "mliis_final_conv_bwd_data_fin", "mliis_chan_split"},
    "op_by_op_dice": set(),
    "darc1_adam": {"mliis_darc1"},
    "aspp": {"mliis_swish_mask_fwd", "mliis_swish_mask_bwd"},
    "bf16_storage": {"mliis_mbconv_dw_fwd_small", "mliis_mbconv_dw_bwd_small", "mliis_dwconv_bn_fwd", "mliis_mbconv_dw_bwd_march"},
    "full_224": {"mliis_conv2d_fwd_x3", "mliis_conv2d_bwd_data_x3", "mliis_weight_shadows"},
    "graph_fomaml_tail": set(),
}

CONFIGS = [
    ("defaults", 64, dict(), False),
    ("op_by_op_dice", 64, dict(small_fused=False, dw_march=False, dice=True, label_smoothing=0.1), False),
    ("darc1_adam", 64, dict(darc1=True, optimizer="adam"), False),
    ("aspp", 64, dict(spatial_pyramid_pooling=True, skip_decoding=True), False),
    ("bf16_storage", 64, dict(matmul_precision="bf16-storage"), False),
    ("full_224", 224, dict(matmul_precision="fp32"), False),
    ("graph_fomaml_tail", 64, dict(), True),
]


def _dc(L, N, seed):
    """Injected drop-connect scales (one dropped sample) for every block that has the site."""
    g = np.random.default_rng(seed)
    out = {}
    for b in L.arch.blocks:
        if b.executed and b.skip:
            out[b.idx] = torch.tensor(np.floor(0.8 + g.random(N)) / 0.8)
    if out:
        out[sorted(out)[-1]][0] = 0.0
    return out


def _poison_grad(L):
    """NaN in every trainable region of arena.grad (the padding is left alone): the step must write every element it reads."""
    A = L.arena
    for p in A.trainable:
        o = A.t_off[p.name]
        A.grad[o:o + p.size].fill_(float("nan"))


def _state(L, N):
    L.synchronize()
    return dict(loss=L.last_loss.clone(), grad=L.arena.grad.clone(), theta=L.arena.theta.clone(), bn=L.export_bn().clone())


def _assert_same(a, b, tag):
    for k in a:
        assert M.bits_equal(a[k], b[k]), "{}: {} differs between the poisoned and the clean learner".format(tag, k)
        if k != "grad":
            assert not torch.isnan(a[k]).any(), "{}: {} is NaN".format(tag, k)


@pytest.mark.parametrize("name,H,kw,graph", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_step_on_poisoned_memory_is_bit_identical(name, H, kw, graph):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import synthetic_task
    N = 8
    x, y = synthetic_task(10, H, seed=2)
    batches = [[0, 1, 2, 3, 4, 5, 6, 7], [7, 6, 5, 4, 3, 2, 1, 0], [1, 3, 5, 7, 9, 0, 2, 4]]
    if graph:
        batches.append([9, 8, 7, 6, 5])          # a FOMAML tail batch of 5 next to the N = 8 plan
    else:
        batches = batches[:2]
    M.reset_guards()
    learners = {}
    reached = M.Reached()
    try:
        for poisoned in (True, False):
            args = dict(image_size=H, seed=3, use_graph=graph, **kw)
            if poisoned:
                with M.poisoned_allocations(), M.record() as r:
                    L = Learner(**args)
                    learners[poisoned] = L
                    L.load_task(x, y)
                    L._plan(N)
                    if graph:
                        L._plan(5)
                    _poison_grad(L)
                    if not graph:    # (eager: what the first step allocates lazily is poisoned too; graph: no hook while capturing)
                        L.inner_step(batches[0], dc_scales=_dc(L, N, 0))
                reached |= r
                calls = list(r.calls)
                with M.record() as r:
                    rest = batches[0 if graph else 1:]
                    for i, idx in enumerate(rest):
                        L.inner_step(idx, dc_scales=None if graph else _dc(L, len(idx), i + (0 if graph else 1)))
                reached |= r
                calls += r.calls
            else:
                L = Learner(**args)
                learners[poisoned] = L
                L.load_task(x, y)
                for i, idx in enumerate(batches):
                    L.inner_step(idx, dc_scales=None if graph else _dc(L, len(idx), i))
        Lp, Lc = learners[True], learners[False]
        _assert_same(_state(Lp, N), _state(Lc, N), name)
        for training in (False, True):
            pp, lp = Lp.predict(x[:3], training=training, return_logits=True)
            pc, lc = Lc.predict(x[:3], training=training, return_logits=True)
            assert M.bits_equal(lp, lc) and torch.equal(pp, pc), "{}: predict(training={}) differs".format(name, training)
            assert not torch.isnan(lp).any()
        M.assert_guards()
        missing = REACHES[name] - reached
        assert not missing, "{} did not reach {}".format(name, sorted(missing))
        if name == "bf16_storage":
            assert Lp.act_dtype == torch.bfloat16
            assert any(t.dtype == torch.bfloat16 for B in Lp.plans[N].blocks for t in B.values() if torch.is_tensor(t)), \
                "no bf16 tensors in the plan"
        if name == "full_224":   # the stream-K and k-split 1x1 plans of config 2 are among the dense convs the step launched
            from mliis_amd import ops
            kinds = set()
            for n, a in calls:
                if n == "mliis_conv2d_fwd":            # (x, ldx, x_scale, wt, bias, border_bias, out, ldy, N, H, W, Cin_total, ci_begin, Cin, Cout, k ...)
                    kinds.add(ops.conv2d_kernel_name(a[8], a[9], a[10], a[13], a[14], a[15]))
                elif n == "mliis_conv2d_fwd_bnin":     # (..., out, ldy, N, H, W, Cin, Cout, ...)
                    kinds.add(ops.conv2d_kernel_name(a[20], a[21], a[22], a[23], a[24], 1))
                elif n.startswith("mliis_conv2d_bwd_data") and not n.endswith("_x3"):   # (dy, lddy, w, out, lddx, N, H, W, Cin, ci_begin, ci_count, Cout, k ...)
                    kinds.add(ops.conv2d_kernel_name(a[5], a[6], a[7], a[11], a[10], a[12]))
            assert any(k.startswith("conv1x1_stream_k") for k in kinds) and any(k.startswith("conv1x1_ksplit_k") for k in kinds), kinds
    finally:
        for L in learners.values():
            L.close()
        M.reset_guards()
