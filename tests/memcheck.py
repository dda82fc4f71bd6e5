"""Poisoned-memory harness of the memory-contract tests (a plain module: tests import it, nothing here is collected).

poisoned_allocations() patches torch.empty / torch.empty_like so that every CUDA float32 / bfloat16 request returns the START of a
larger allocation: the requested region is NaN and a guard band of a distinctive quiet-NaN bit pattern follows it.  A kernel that
reads an output or workspace before writing it sees NaN; one that writes past the end of its buffer changes the guard, which
assert_guards() compares bitwise and reports by the shape of the allocation.  CPU tensors (the float64 oracle) and integer dtypes are
left alone.  guarded_input() / nan_gap_view() do the same for inputs and channel-slice views, snapshot() checks that inputs are left
bit-identical, record() lists the C entry points a case really reached (lib.trace).

COVERED / EXEMPT: the manifest of include/mliis_hip.h's entry points.  Every entry point is either reached by a memory-contract case
(tests/test_memory_contract_gpu.py, tests/test_step_poisoned_gpu.py: each case asserts what it reached) or exempt with a reason;
tests/test_memory_contract_cpu.py checks that the two lists together are exactly the header's set.
"""
from __future__ import annotations

import contextlib

import torch

# quiet NaNs with a payload no arithmetic produces (a kernel's NaN result is 0x7fc00000 / 0x7fc0 or a propagated input payload)
GUARD_F32 = 0x7FD1A5E3
GUARD_BF16 = 0x7FE5
GUARD_MAX_ELEMS = 1 << 20          # 4 MB of float32 guard at most; at least the allocation itself below that
GUARD_MIN_ELEMS = 1024


def _int_view(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _pattern(dtype) -> int:
    return GUARD_BF16 if dtype == torch.bfloat16 else GUARD_F32


def guard_elems(n: int) -> int:
    return min(max(int(n), GUARD_MIN_ELEMS), GUARD_MAX_ELEMS)


def fill_guard(t: torch.Tensor) -> torch.Tensor:
    _int_view(t).fill_(_pattern(t.dtype))
    return t


class _Registry:
    def __init__(self):
        self.entries = []          # (label, region): region must hold its dtype's guard pattern

    def add(self, label, region):
        self.entries.append((label, region))

    def broken(self):
        bad = []
        for label, region in self.entries:
            if region.numel() and not bool((_int_view(region) == _pattern(region.dtype)).all()):
                bad.append(label)
        return bad


_REG = _Registry()


def _guarded(numel: int, dtype, device, label) -> torch.Tensor:
    """[numel] NaN followed by its guard band (registered); returns the flat head."""
    g = guard_elems(numel)
    base = torch.zeros(numel + g, dtype=dtype, device=device)   # (torch.zeros: never the patched allocator)
    fill_guard(base[numel:])
    base[:numel].fill_(float("nan"))
    _REG.add(label, base[numel:])
    return base[:numel]


def _size_of(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


def _poisonable(dtype, device) -> bool:
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    return device is not None and torch.device(device).type == "cuda"


@contextlib.contextmanager
def poisoned_allocations():
    """While active, CUDA float32 / bfloat16 torch.empty / torch.empty_like return NaN heads of guarded allocations; the default
    Workspace of mliis_amd.ops is re-created under the hook.  Both functions and the workspace are restored on every exit path."""
    from mliis_amd import ops
    real_empty, real_like = torch.empty, torch.empty_like

    def empty(*size, dtype=None, device=None, out=None, memory_format=None, **kw):
        dt = torch.get_default_dtype() if dtype is None else dtype
        if out is not None or kw.get("pin_memory") or memory_format not in (None, torch.contiguous_format) or not _poisonable(dt, device):
            extra = dict(kw, out=out) if out is not None else kw
            if memory_format is not None:
                extra["memory_format"] = memory_format
            return real_empty(*size, dtype=dtype, device=device, **extra)
        shape = _size_of(size)
        n = 1
        for s in shape:
            n *= s
        t = _guarded(n, dt, device, "empty{} {}".format(shape, dt)).view(shape)
        if kw.get("requires_grad"):
            t.requires_grad_(True)
        return t

    def empty_like(src, *, dtype=None, device=None, memory_format=None, **kw):
        dt = src.dtype if dtype is None else dtype
        dv = src.device if device is None else device
        if kw or memory_format not in (None, torch.preserve_format, torch.contiguous_format) or not _poisonable(dt, dv) or \
                (memory_format is None and not src.is_contiguous()):
            extra = dict(kw)
            if memory_format is not None:
                extra["memory_format"] = memory_format
            return real_like(src, dtype=dtype, device=device, **extra)
        return empty(tuple(src.shape), dtype=dt, device=dv)

    saved_ws = ops._default_ws
    torch.empty, torch.empty_like = empty, empty_like
    ops._default_ws = None
    try:
        yield _REG
    finally:
        torch.empty, torch.empty_like = real_empty, real_like
        ops._default_ws = saved_ws


def reset_guards():
    """Forget the guards registered so far (a test starts with its own registry)."""
    _REG.entries = []


def assert_guards():
    """Every guard band registered since reset_guards() still holds its bit pattern; names the allocations whose guard changed."""
    torch.cuda.synchronize()
    bad = _REG.broken()
    assert not bad, "guard band overwritten behind: " + ", ".join(bad[:12]) + (" (+{} more)".format(len(bad) - 12) if len(bad) > 12 else "")


# ------------------------------------------------------------------------------------------------ inputs and views
def guarded_input(t: torch.Tensor) -> torch.Tensor:
    """A dense device copy of t that ENDS where a guard band begins (and starts right after another): reads past its last element
    see NaN; writes there break the guard."""
    t = t.to(device="cuda", dtype=t.dtype if t.dtype in (torch.float32, torch.bfloat16) else torch.float32).contiguous()
    n = t.numel()
    g = guard_elems(n)
    base = torch.zeros(g + n + g, dtype=t.dtype, device=t.device)
    fill_guard(base)
    base[g:g + n] = t.reshape(-1)
    label = "input{} {}".format(tuple(t.shape), t.dtype)
    _REG.add(label + " (front)", base[:g])
    _REG.add(label + " (back)", base[g + n:])
    return base[g:g + n].view(t.shape)


def nan_gap_view(t: torch.Tensor, pad: int, lead: int = 0) -> torch.Tensor:
    """A channel-slice view [..., lead : lead + C] of a guarded [..., lead + C + pad] buffer holding t; the gap channels hold the guard
    pattern (NaN) and are registered: a kernel that ignores the row stride reads NaN, one that writes into the gap breaks a guard."""
    t = t.to(device="cuda", dtype=t.dtype if t.dtype in (torch.float32, torch.bfloat16) else torch.float32)
    C = t.shape[-1]
    wide_shape = tuple(t.shape[:-1]) + (lead + C + pad,)
    n = 1
    for s in wide_shape:
        n *= s
    g = guard_elems(n)
    base = torch.zeros(n + g, dtype=t.dtype, device=t.device)
    fill_guard(base)
    wide = base[:n].view(wide_shape)
    wide[..., lead:lead + C] = t
    label = "view{} ld {} {}".format(tuple(t.shape), lead + C + pad, t.dtype)
    if pad:
        _REG.add(label + " (gap)", wide[..., lead + C:])
    if lead:
        _REG.add(label + " (lead gap)", wide[..., :lead])
    _REG.add(label + " (tail)", base[n:])
    return wide[..., lead:lead + C]


def guarded_out_short(shape, dtype=torch.float32, short=1):
    """A dense tensor of `shape` with its last dimension `short` smaller, followed by a guard of at least one full `shape`: the wrong
    caller out= of the wrapper-contract tests.  A wrapper that does not refuse it writes into the guard, never past the allocation."""
    bad = tuple(shape[:-1]) + (shape[-1] - short,)
    full = 1
    for s in shape:
        full *= s
    n = 1
    for s in bad:
        n *= s
    base = torch.zeros(n + max(guard_elems(full), full), dtype=dtype, device="cuda")
    fill_guard(base[n:])
    base[:n].fill_(float("nan"))
    _REG.add("short out{} {}".format(bad, dtype), base[n:])
    return base[:n].view(bad)


def guarded_wrong_dtype(shape, dtype):
    """A dense `dtype` tensor of `shape` laid at the start of a float32 buffer that holds one full float32 output of `shape`, with a
    guard behind it: a wrapper that does not refuse the dtype writes float32 values inside that buffer, never past it."""
    full = 1
    for s in shape:
        full *= s
    base = torch.zeros(full + guard_elems(full), dtype=torch.float32, device="cuda")
    fill_guard(base[full:])
    _REG.add("wrong-dtype out{} {}".format(tuple(shape), dtype), base[full:])
    n_bytes = full * torch.tensor([], dtype=dtype).element_size()
    assert n_bytes <= 4 * full
    return base.view(torch.uint8)[:n_bytes].view(dtype).view(tuple(shape))


class FixedWorkspace:
    """A Workspace whose get() hands out exactly `buf`, whatever is asked: the library sees buf.numel() as the capacity (the grow-only
    Workspace would replace a buffer that is too small)."""

    def __init__(self, buf):
        self.buf = buf

    def get(self, floats: int) -> torch.Tensor:
        return self.buf


class Snapshot:
    def __init__(self, tensors):
        torch.cuda.synchronize()
        self.items = [(t, _int_view(t).clone()) for t in tensors if t is not None and t.dtype in (torch.float32, torch.bfloat16)]

    def assert_unchanged(self):
        torch.cuda.synchronize()
        for i, (t, bits) in enumerate(self.items):
            assert torch.equal(_int_view(t), bits), "input {} {} was written by the call".format(i, tuple(t.shape))


def snapshot(*inputs) -> Snapshot:
    return Snapshot(inputs)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_int_view(a.contiguous()), _int_view(b.contiguous()))


# ------------------------------------------------------------------------------------------------ entry-point recorder
class Reached(set):
    """Entry-point names; .calls keeps the (name, ctypes args) of every call."""
    calls = ()


@contextlib.contextmanager
def record():
    """Names of the mliis_* entry points called (through lib.call) while active: a set that fills when the block ends."""
    from mliis_amd._lib import lib
    prev = lib.trace
    trace = []
    reached = Reached()
    reached.calls = trace
    lib.trace = trace
    try:
        yield reached
    finally:
        lib.trace = prev
        reached.update(name for name, _ in trace)
        if prev is not None:
            prev.extend(trace)


# ------------------------------------------------------------------------------------------------ coverage manifest
# entry points that run work on the device and are reached by a memory-contract case (each case asserts its own subset)
COVERED = {
    "mliis_stem_conv_fwd", "mliis_stem_conv_fwd_stats", "mliis_stem_conv_bwd_filter",
    "mliis_dwconv_fwd", "mliis_dwconv_bwd_data", "mliis_dwconv_bwd_data_bn", "mliis_dwconv_bwd_filter",
    "mliis_dwconv_bn_fwd", "mliis_dwconv_bn_bwd", "mliis_mbconv_dw_bwd_march",
    "mliis_mbconv_dw_fwd_small", "mliis_mbconv_dw_bwd_small",
    "mliis_conv2d_fwd", "mliis_conv2d_fwd_bnin", "mliis_conv2d_bwd_data", "mliis_conv2d_bwd_data_bn", "mliis_conv2d_bwd_data_gate",
    "mliis_conv2d_bwd_filter", "mliis_conv2d_bwd_filter_batched",
    "mliis_conv2d_fwd_x3", "mliis_conv2d_bwd_data_x3", "mliis_x3_pack_weights",
    "mliis_transpose_weights", "mliis_weight_shadows", "mliis_weight_shadows_rng",
    "mliis_head_ce_fused", "mliis_rsd_concat_pool", "mliis_rsd_pool_fwd", "mliis_rsd_pool_bwd",
    "mliis_bn_stats", "mliis_bn_apply", "mliis_bn_stats_partial", "mliis_bn_apply_fused", "mliis_bn_bwd",
    "mliis_bn_apply_fused_pair", "mliis_bn_bwd_pair", "mliis_colsum",
    "mliis_se_mlp_fwd", "mliis_se_mlp_bwd", "mliis_se_bn_bwd_sums", "mliis_se_mlp_bwd_bn", "mliis_se_wgrad_batched",
    "mliis_chan_affine", "mliis_chan_split", "mliis_swish_mask_fwd", "mliis_swish_mask_bwd",
    "mliis_resize_bilinear_fwd", "mliis_resize_bilinear_bwd",
    "mliis_final_conv_fwd", "mliis_final_conv_bwd_data", "mliis_final_conv_bwd_data_fin", "mliis_final_conv_bwd_filter",
    "mliis_softmax_ce", "mliis_darc1", "mliis_sgd_fused", "mliis_adam_b1zero_fused", "mliis_axpby", "mliis_lincomb",
    "mliis_copy_words", "mliis_fold_batched",
}

_W = "capacity tested at the queried size and one less by test_memory_contract_gpu.test_workspace_queries_at_the_queried_size_and_one_less"
_P = "capacity tested at the queried size and one block less by test_memory_contract_gpu.test_capacities_at_the_queried_size_and_one_block_less"

EXEMPT = {
    "mliis_version": "query: returns a constant, touches no memory",
    "mliis_last_error": "query: the library's error string",
    "mliis_stem_conv_fwd_stats_floats": "size query, no device work; " + _P,
    "mliis_stem_conv_bwd_filter_workspace_floats": "size query, no device work; " + _W,
    "mliis_dwconv_bwd_filter_workspace_floats": "size query, no device work; " + _W,
    "mliis_dwconv_bn_fwd_blocks": "block query, no device work; " + _P,
    "mliis_dwconv_bn_supported": "shape predicate, no device work",
    "mliis_dwconv_bn_bwd_blocks": "block query, no device work; " + _P,
    "mliis_mbconv_dw_small_supported": "shape predicate, no device work",
    "mliis_mbconv_dw_small_group_width": "planner query, no device work",
    "mliis_conv2d_workspace_floats": "size query, no device work; " + _W,
    "mliis_conv2d_plan": "planner query, no device work",
    "mliis_conv1x1_occupancy": "planner query, no device work",
    "mliis_conv2d_kernel_name": "planner query, no device work",
    "mliis_head_ce_fused_supported": "shape predicate, no device work",
    "mliis_head_ce_fused_workspace_floats": "size query, no device work; " + _W,
    "mliis_conv2d_fwd_bnin_ok": "shape predicate, no device work",
    "mliis_rsd_concat_pool_floats": "size query, no device work; " + _P,
    "mliis_rsd_pool_bwd_workspace_floats": "size query, no device work; " + _W,
    "mliis_x3_image_bytes": "size query, no device work; NOT capacity-tested: the images of all convs share one packed byte allocation (X3Images); they are read under poison by the x3 parity case only",
    "mliis_x3_image_blocks": "grid query, no device work; NOT capacity-tested (see mliis_x3_image_bytes)",
    "mliis_conv2d_x3_workspace_floats": "size query, no device work; " + _W,
    "mliis_conv2d_x3_plan": "planner query, no device work",
    "mliis_conv2d_bwd_filter_workspace_floats": "size query, no device work; " + _W,
    "mliis_conv2d_bwd_filter_plan": "planner query, no device work",
    "mliis_colreduce_workspace_floats": "size query, no device work; " + _W + " (bn_stats, bn_bwd, colsum, final_conv_bwd_filter) and " + _P + " (bn_stats_partial)",
    "mliis_bn_bwd_dxsum_floats": "size query, no device work; " + _W,
    "mliis_se_bn_bwd_sums_floats": "size query, no device work; " + _P,
    "mliis_softmax_ce_workspace_floats": "size query, no device work; " + _W,
    "mliis_fold_tile_outputs": "constant query, no device work",
    "mliis_rng_masks": "its device counter and outputs are covered by test_ops_gpu.test_rng_masks_are_philox_and_advance_per_launch",
    "mliis_augment_stage": "writes whole images of the resident task; covered bitwise by tests/test_augment_gpu.py",
    "mliis_graph_begin_capture": "HIP graph control, no kernel memory of its own",
    "mliis_graph_end_capture": "HIP graph control, no kernel memory of its own",
    "mliis_graph_launch": "replays the captured step: covered by the graph variant of tests/test_step_poisoned_gpu.py",
    "mliis_graph_destroy": "HIP graph control, no kernel memory of its own",
}


def guarded_buffer(floats: int, fill=float("nan"), dtype=torch.float32) -> torch.Tensor:
    """A flat device buffer of exactly `floats` elements (filled with `fill`) followed by a registered guard band: a capacity passed
    to the library as buffer.numel() that the library must not exceed."""
    n = int(floats)
    base = torch.zeros(n + guard_elems(n), dtype=dtype, device="cuda")
    fill_guard(base[n:])
    base[:n].fill_(fill)
    _REG.add("buffer[{}] {}".format(n, dtype), base[n:])
    return base[:n]
