"""The inner loop's gradient clipping on the device: mliis_clip_apply (csrc/clip.hip, libmliis_clip.so) through ops.clip_apply against numpy
in float64 over the counted elements -- norms, scales, the one fp32 product per element, padding, non-finite gradients, determinism, the
ring row and the cursor, the memory contract, the argument errors -- then Learner(grad_clip=...) against an unclipped twin, the fused
optimizer ops and a graph-free run, Gecko over a lane, the step log beside it and a task with a NaN pixel."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import memcheck

pytestmark = pytest.mark.gpu

H = 64
SENTINEL = 0x5A5A5A5A
FLT_MIN = float(np.finfo(np.float32).tiny)
CLIPPED, BYPASSED = 1, 2


def _ch():
    from mliis_amd._lib import clip_lib
    return 4 * clip_lib.size("mliis_clip_chunk_quads")


def _offsets(sizes):
    off, o = [], 0
    for s in sizes:
        off.append(o)
        o += (s + 3) // 4 * 4
    return off, o


def _arena_sizes(n):
    """Tensor sizes of an arena of n floats: 4 -- one tensor of 3; 1028 -- small odd tensors; 262148 -- a one-element tensor, exactly one
    chunk, one chunk + 1 quad and a tensor of 14 chunks whose last is short."""
    CH = _ch()
    sizes = {4: [3], 1028: [1, 5, 255, 257, 499], 262148: [CH, CH + 4, 1, 262148 - 2 * CH - 8 - 2]}[n]
    assert _offsets(sizes)[1] == n
    return sizes


def _b0_sizes():
    from mliis_amd import spec
    arch = spec.derive("efficientnet-b0", 224, [2, 4], 0.0, False, skip_decoding=False)
    sizes = [p.size for p in spec.param_table(arch) if p.trainable]
    assert len(sizes) == 169
    return sizes


def _values(sizes, seed, pad=1e30):
    """(g, theta): N(0, 1) gradients and N(0, 0.1) parameters; every padding float of both holds `pad`."""
    off, n = _offsets(sizes)
    r = np.random.default_rng(seed)
    g, th = r.standard_normal(n).astype(np.float32), (0.1 * r.standard_normal(n)).astype(np.float32)
    for t, s in enumerate(sizes):
        for a in (g, th):
            a[off[t] + s:off[t] + (s + 3) // 4 * 4] = pad
    return g, th


def _norm64(v):
    fin = np.isfinite(v)
    v64 = v[fin].astype(np.float64)
    return float(np.sqrt(np.sum(v64 * v64))), int((~fin).sum())


def _reference(mode, sizes, g, th, threshold, eps):
    """Per record from float64 numpy over the counted elements: (norm64, ref64, nonfinite, clipped, bypassed, [tensor indices])."""
    off, _ = _offsets(sizes)
    parts = [(g[off[t]:off[t] + s], th[off[t]:off[t] + s]) for t, s in enumerate(sizes)]
    bypassed = any(_norm64(gv)[1] for gv, _ in parts)
    thr, e = float(np.float32(threshold)), float(np.float32(eps))
    if mode == "norm":
        allg = np.concatenate([gv for gv, _ in parts])
        norm, nf = _norm64(allg)
        return [(norm, thr, nf, (not bypassed) and norm > thr, bypassed, list(range(len(sizes))))]
    out = []
    for t, (gv, tv) in enumerate(parts):
        norm, nf = _norm64(gv)
        ref = thr * max(_norm64(tv)[0], e)
        out.append((norm, ref, nf, (not bypassed) and norm > ref, bypassed, [t]))
    return out


def _within_one_spacing(got, want64, what):
    want = np.float32(want64)
    print("{}: device {!r}, float64 numpy rounded to f32 {!r}".format(what, got, want))
    assert abs(float(got) - float(want)) <= float(np.spacing(want)), what


def _assert_product(out, g, scale, what):
    """out == g * scale as ONE numpy float32 product, bit for bit; where that product is below FLT_MIN the IEEE subnormal (which is what
    numpy forms, and what include/mliis_clip.h says the kernel gives) or a zero of its sign is accepted."""
    with np.errstate(over="ignore", under="ignore"):
        want = g * np.float32(scale)
    assert want.dtype == np.float32
    same = out.view(np.uint32) == want.view(np.uint32)
    tiny = np.abs(want) < FLT_MIN
    zero = (out == 0) & (np.signbit(out) == np.signbit(want))
    assert bool((same | (tiny & zero)).all()), (what, int((~(same | (tiny & zero))).sum()))


def _ring(capacity, R):
    ring = memcheck.guarded_buffer(capacity * R * 8, fill=0.0).view(torch.int32).view(capacity, R, 8)
    ring.fill_(SENTINEL)
    return ring


def _cursor(value):
    c = memcheck.guarded_buffer(4, fill=0.0).view(torch.int32)[:1]
    c.fill_(value)
    return c


def _records(ring):
    from mliis_amd import clip
    torch.cuda.synchronize()
    return ring.cpu().numpy().view(clip.RECORD_DTYPE).reshape(ring.shape[0], ring.shape[1])


class _Case:
    """One arena on the device with guard bands round every buffer; apply() runs ops.clip_apply and returns (gradient after, its row)."""

    def __init__(self, sizes, g_h, th_h, capacity=2):
        from mliis_amd import ops
        self.sizes, self.g_h, self.th_h = sizes, g_h, th_h
        self.off, self.n = _offsets(sizes)
        self.theta = memcheck.guarded_input(torch.from_numpy(th_h))
        self.table = ops.clip_table(sizes, self.theta.device)
        assert self.table.n == self.n and self.table.T == len(sizes)
        self.ws = memcheck.guarded_buffer(ops.clip_workspace(self.table).numel(), fill=0.0).view(torch.int32)
        self.ws.fill_(SENTINEL)                          # (its contents before a launch do not matter)
        self.cursor, self.capacity = _cursor(0), capacity
        self.snap = memcheck.snapshot(self.theta, self.table.chunks.view(torch.float32), self.table.segs.view(torch.float32))

    def apply(self, mode, threshold, eps=1e-3, g_h=None):
        from mliis_amd import ops
        g = memcheck.guarded_input(torch.from_numpy(self.g_h if g_h is None else g_h))
        ring = _ring(self.capacity, len(self.sizes) if mode == "ratio" else 1)
        before = int(self.cursor.item())
        assert ops.clip_apply(g, self.theta, self.table, self.ws, self.cursor, mode, threshold, eps, out=ring) is ring
        rec = _records(ring)
        row = before % self.capacity
        others = [k for k in range(self.capacity) if k != row]
        assert bool((ring[others] == SENTINEL).all()) and int(self.cursor.item()) == before + 1     # one row; the cursor moved by one
        return g.cpu().numpy(), rec[row]

    def check(self, mode, threshold, eps, out, rec, g_h=None):
        """The records against _reference and the arena against the recorded scales; returns the reference."""
        g_h = self.g_h if g_h is None else g_h
        want = _reference(mode, self.sizes, g_h, self.th_h, threshold, eps)
        assert len(rec) == len(want)
        for r, (norm, ref, nf, clipped, bypassed, tensors) in enumerate(want):
            what = "{} n={} record {}".format(mode, self.n, r)
            _within_one_spacing(rec["g_l2"][r], norm, what + " g_l2")
            _within_one_spacing(rec["ref"][r], ref, what + " ref")
            assert int(rec["nonfinite"][r]) == nf and int(rec["flags"][r]) == (CLIPPED if clipped else 0) | (BYPASSED if bypassed else 0), what
            assert not rec["zero"][r].any()
            if clipped:
                _within_one_spacing(rec["scale"][r], ref / norm, what + " scale")
                assert 0.0 < float(rec["scale"][r]) <= 1.0
            else:
                assert rec["scale"][r].tobytes() == np.float32(1.0).tobytes(), what
            for t in tensors:                            # every float of the tensor's quads, its padding too
                lo, hi = self.off[t], self.off[t] + (self.sizes[t] + 3) // 4 * 4
                if clipped:
                    _assert_product(out[lo:hi], g_h[lo:hi], rec["scale"][r], what)
                else:
                    assert out[lo:hi].tobytes() == g_h[lo:hi].tobytes(), what
        return want

    def done(self):
        self.snap.assert_unchanged()
        memcheck.assert_guards()


@pytest.mark.parametrize("n", [4, 1028, 262148, "b0"])
def test_both_modes_against_float64_numpy_with_padding_and_guards(n):
    sizes = _b0_sizes() if n == "b0" else _arena_sizes(n)
    g_h, th_h = _values(sizes, seed=3)                   # 1e30 in every padding float: it enters no norm
    memcheck.reset_guards()
    case = _Case(sizes, g_h, th_h)
    norm = _norm64(np.concatenate([g_h[o:o + s] for o, s in zip(case.off, sizes)]))[0]
    # global norm: clipped at half the norm, untouched at twice the norm
    out, rec = case.apply("norm", 0.5 * norm)
    want = case.check("norm", 0.5 * norm, 1e-3, out, rec)
    assert want[0][3] and rec["ref"][0].tobytes() == np.float32(0.5 * norm).tobytes()
    out, rec = case.apply("norm", 2.0 * norm)
    assert not case.check("norm", 2.0 * norm, 1e-3, out, rec)[0][3] and out.tobytes() == g_h.tobytes() and not np.isnan(out).any()
    # per tensor: ||g_t|| / ||theta_t|| is about 10 (or ||g_t|| / eps where a tensor is tiny), so LAMBDA = 5 clips every tensor and
    # LAMBDA = 40 clips only those whose ratio the draw left above it; at least one of each kind where there is more than one tensor
    for lam in (5.0, 40.0):
        out, rec = case.apply("ratio", lam, 1e-3)
        case.check("ratio", lam, 1e-3, out, rec)
    # determinism: two calls on equal inputs give equal bits
    a, ra = case.apply("ratio", 5.0, 1e-3)
    b, rb = case.apply("ratio", 5.0, 1e-3)
    assert a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes()
    a, ra = case.apply("norm", 0.5 * norm)
    b, rb = case.apply("norm", 0.5 * norm)
    assert a.tobytes() == b.tobytes() and ra.tobytes() == rb.tobytes()
    case.done()


def test_ratio_mode_clips_one_tensor_beside_one_it_leaves_and_floors_zero_parameters():
    CH = _ch()
    sizes = [300, CH + 5, 1, 64, 7]
    off, n = _offsets(sizes)
    g_h, th_h = _values(sizes, seed=5)
    th_h[off[0]:off[0] + 300] *= 100.0                   # tensor 0: ||theta|| ~ 170, LAMBDA ||theta|| far above ||g|| ~ 17: left alone
    th_h[off[3]:off[3] + 64] = 0.0                       # tensor 3: theta all zero, ref = LAMBDA * eps
    th_h[off[4]:off[4] + 7] = 0.0
    g_h[off[4]:off[4] + 7] = 1e-6                        # tensor 4: zero parameters and a gradient below the floor: left alone
    memcheck.reset_guards()
    case = _Case(sizes, g_h, th_h)
    out, rec = case.apply("ratio", 0.5, 1e-2)
    want = case.check("ratio", 0.5, 1e-2, out, rec)
    assert [w[3] for w in want] == [False, True, True, True, False]
    assert rec["ref"][3].tobytes() == np.float32(float(np.float32(0.5)) * float(np.float32(1e-2))).tobytes() == rec["ref"][4].tobytes()
    assert out[off[2]] == np.float32(g_h[off[2]] * rec["scale"][2])             # the one-element tensor
    # an all-zero gradient: bit-identical, scale exactly 1, flag clear, no NaN -- in both modes
    zero = np.zeros(n, dtype=np.float32)
    for mode, thr in (("norm", 1.0), ("ratio", 0.5)):
        out, rec = case.apply(mode, thr, 1e-2, g_h=zero)
        assert out.tobytes() == zero.tobytes() and not rec["flags"].any() and not rec["g_l2"].any() and not rec["nonfinite"].any()
        assert rec["scale"].tobytes() == np.ones(len(rec), dtype=np.float32).tobytes()
    case.done()


def test_a_non_finite_gradient_is_left_bit_for_bit_and_every_record_is_bypassed():
    CH = _ch()
    sizes = [300, 2 * CH + 9, 64]
    off, n = _offsets(sizes)
    g_h, th_h = _values(sizes, seed=7)
    g_h[off[1] + 3], g_h[off[1] + CH + 17], g_h[off[1] + 2 * CH + 8] = np.nan, np.inf, -np.inf       # one in each chunk of tensor 1
    g_h[off[1] + 5] = np.float32(np.uint32(0x7FA00001).view(np.float32))                              # a signalling NaN keeps its payload
    memcheck.reset_guards()
    case = _Case(sizes, g_h, th_h)
    for mode, thr in (("norm", 1e-3), ("ratio", 1e-3)):                                               # bounds every finite tensor exceeds
        out, rec = case.apply(mode, thr)
        assert out.tobytes() == g_h.tobytes()
        assert (rec["flags"] == BYPASSED).all() and rec["scale"].tobytes() == np.ones(len(rec), dtype=np.float32).tobytes()
        assert rec["nonfinite"].tolist() == ([4] if mode == "norm" else [0, 4, 0])
        case.check(mode, thr, 1e-3, out, rec)
    case.done()


def test_three_calls_land_in_the_right_rows_and_the_cursor_reads_three():
    from mliis_amd import ops
    sizes = [5, 300]
    g_h, th_h = _values(sizes, seed=9)
    memcheck.reset_guards()
    for capacity in (4, 2):
        case = _Case(sizes, g_h, th_h, capacity=capacity)
        ring, g = _ring(capacity, 1), memcheck.guarded_input(torch.from_numpy(g_h))
        norms = []
        for k in range(3):                               # each call halves the gradient: rows hold 1, 1/2, 1/4 of the first norm
            norms.append(_norm64(g.cpu().numpy()[np.isfinite(g_h) & (np.abs(g_h) < 1e29)])[0])
            ops.clip_apply(g, case.theta, case.table, case.ws, case.cursor, "norm", 0.5 * norms[-1], out=ring)
        rec = _records(ring)
        assert int(case.cursor.item()) == 3
        for k in range(3):
            if k >= 3 - capacity:                        # (capacity 2: row 0 was overwritten by the third call)
                _within_one_spacing(rec["g_l2"][k % capacity, 0], norms[k], "capacity {} call {}".format(capacity, k))
        if capacity == 4:
            assert bool((ring[3] == SENTINEL).all())
        case.done()


def test_bad_arguments_are_refused_before_any_launch():
    from mliis_amd import layerlog as LL
    from mliis_amd import ops
    from mliis_amd._lib import MliisError, clip_lib
    sizes = [5, 300, 64]
    _, n = _offsets(sizes)
    memcheck.reset_guards()
    g, th = torch.randn(n + 4, device="cuda"), torch.randn(n + 4, device="cuda")
    g0 = g.clone()
    table = ops.clip_table(sizes, g.device)
    T, nch = table.T, table.nchunks
    ring, cursor = _ring(2, T), _cursor(0)
    need = clip_lib.size("mliis_clip_workspace_bytes", nch, T)
    ws = memcheck.guarded_buffer(need // 4 + 4, fill=0.0).view(torch.int32)
    ws.fill_(SENTINEL)
    raw = clip_lib.load().mliis_clip_apply
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)   # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    good = [1, p(g), p(th), n, p(table.chunks), nch, p(table.segs), T, 0.5, 1e-3, p(ws), need, p(ring), 2, p(cursor), st]
    ARG, ALIGN = -1, -3
    cases = []
    for i in (1, 2, 4, 6, 10, 12, 14):                    # every pointer null in turn (ratio mode: theta too)
        cases.append((ARG, good[:i] + [None] + good[i + 1:]))
    for mode in (-1, 2):
        cases.append((ARG, [mode] + good[1:]))
    for bad_n in (0, -4, n + 2, 3):
        cases.append((ARG, good[:3] + [bad_n] + good[4:]))
    for bad_t in (0, -1, nch + 1):                        # no tensor; more tensors than chunks
        cases.append((ARG, good[:7] + [bad_t] + good[8:]))
    for bad_c in (0, T - 1, n // 4 + 1):                  # fewer chunks than tensors; more chunks than quads
        cases.append((ARG, good[:5] + [bad_c] + good[6:]))
    for cap in (0, -1):
        cases.append((ARG, good[:13] + [cap] + good[14:]))
    cases.append((ARG, good[:11] + [need - 1] + good[12:]))          # a workspace one byte short
    for bad in (0.0, -1.0, float("nan"), float("inf")):   # a threshold or an eps that is not finite and positive
        cases.append((ARG, good[:8] + [bad] + good[9:]))
        cases.append((ARG, good[:9] + [bad] + good[10:]))
        cases.append((ARG, [0] + good[1:8] + [bad] + good[9:]))
    for i, t in ((1, g), (2, th), (4, table.chunks), (6, table.segs), (10, ws), (12, ring)):
        cases.append((ALIGN, good[:i] + [p(t, 4)] + good[i + 1:]))
    cases.append((ALIGN, good[:14] + [p(cursor, 2)] + good[15:]))
    for code, args in cases:
        assert raw(*args) == code, args
        assert clip_lib.load().mliis_clip_last_error().startswith(b"clip_apply:")
    torch.cuda.synchronize()
    assert bool((ring == SENTINEL).all()) and bool((ws == SENTINEL).all()) and int(cursor.item()) == 0 and torch.equal(g, g0)   # nothing ran
    # the wrapper: tensors of the wrong kind, size or place, a wrong out=, a table that is none, values that are not positive
    ok = dict(grad=g[:n], theta=th[:n], table=table, ws=ws, cursor=cursor, mode="ratio", threshold=0.5, out=ring)
    for change in (dict(grad=g[:n - 4]), dict(theta=th[:n + 4]), dict(grad=g[::2][:n // 2]), dict(grad=g[:n].double()), dict(grad=g[:n].cpu()),
                   dict(theta=None), dict(table=(table.chunks, table.segs)), dict(ws=ws[:need // 4 - 1]), dict(ws=ws.to(torch.int64)),
                   dict(cursor=torch.zeros(2, dtype=torch.int32, device="cuda")), dict(cursor=torch.zeros(1, device="cuda")), dict(cursor=None),
                   dict(out=torch.zeros(2, T + 1, 8, dtype=torch.int32, device="cuda")), dict(out=torch.zeros(2, 1, 8, dtype=torch.int32, device="cuda")),
                   dict(out=torch.zeros(2, T, 8, dtype=torch.float32, device="cuda")), dict(out=torch.zeros(2, T, 8, dtype=torch.int32)),
                   dict(out=ring, capacity=3), dict(out=None), dict(out=None, capacity=0), dict(mode="both"), dict(threshold=0.0),
                   dict(threshold=float("nan")), dict(eps=-1.0), dict(eps=float("inf"))):
        with pytest.raises(MliisError):
            ops.clip_apply(**dict(ok, **change))
    # tables are validated on the host before they are uploaded
    t = LL.chunk_table(sizes, _ch() // 4)
    for chunks, segs, nn in ((t.chunks, t.segs, t.n - 4), (t.chunks[:-1], t.segs, t.n), (t.chunks, t.segs[::-1].copy(), t.n)):
        with pytest.raises(MliisError, match="clip_table"):
            ops.clip_table(None, g.device, chunks=chunks, segs=segs, n=nn)
    with pytest.raises(MliisError):
        ops.clip_table(sizes, "cpu")
    torch.cuda.synchronize()
    assert bool((ring == SENTINEL).all()) and bool((ws == SENTINEL).all()) and torch.equal(g, g0)
    fresh = ops.clip_apply(g[:n], None, table, ws, cursor, "norm", 1e9, capacity=3)     # and the form that allocates the ring; theta unused
    assert tuple(fresh.shape) == (3, 1, 8) and fresh.dtype == torch.int32 and bool(fresh[0].any()) and not bool(fresh[1:].any())
    assert torch.equal(g, g0)
    memcheck.assert_guards()


# ------------------------------------------------------------------------------------------------ the learner
BATCHES = [[0, 1], [2, 3, 0], [1, 2, 3, 0], [3, 0]]
_TWINS = {}


def _learner(optimizer="sgd", **kw):
    from mliis_amd.learner import Learner
    kw = dict(dict(image_size=H, rsd=[2, 4], drop_connect=False, optimizer=optimizer, seed=5, use_graph=True, learning_rate=5e-3), **kw)
    return Learner(**kw)


def _task(seed=11):
    from mliis_amd import metaseg
    return metaseg.synthetic_task(4, H, seed=seed)


def _twin(optimizer):
    """An unclipped learner's first step on BATCHES[0], computed once per optimizer and left unchanged: the initial parameter arena, the
    gradient arena after the step, the gradient's norm through gradients_packed(), and per tensor ||g_t|| / ||theta_t|| in float64."""
    if optimizer not in _TWINS:
        L = _learner(optimizer)
        L.load_task(*_task())
        torch.cuda.synchronize()
        theta0 = L.arena.theta.clone()
        L.inner_step(BATCHES[0])
        torch.cuda.synchronize()
        packed = L.gradients_packed().cpu().numpy()
        assert np.isfinite(packed).all()
        g, th = L.arena.grad.cpu().numpy(), theta0.cpu().numpy()
        ratios = []
        for p in L.arena.trainable:
            o = L.arena.t_off[p.name]
            ratios.append((_norm64(g[o:o + p.size])[0], _norm64(th[o:o + p.size])[0]))
        _TWINS[optimizer] = dict(theta0=theta0, grad=L.arena.grad.clone(), norm=_norm64(packed)[0], ratios=ratios, theta1=L.arena.theta.clone())
        L.close()
    return _TWINS[optimizer]


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_a_bound_far_above_any_norm_equals_the_unclipped_learner_bit_for_bit(optimizer):
    plain = _learner(optimizer)
    far = [_learner(optimizer, grad_clip=("norm", 1e30)), _learner(optimizer, grad_clip=("ratio", 1e30, 1e-3), clip_log=8)]
    assert far[0].clip_log == 64 and tuple(far[0]._clip_ring.shape) == (64, 1, 8) and tuple(far[1]._clip_ring.shape) == (8, len(plain.arena.trainable), 8)
    x, y = _task()
    for ln in [plain] + far:
        ln.load_task(x, y)
    for b in BATCHES:                                     # four steps: eager, capture, replays where the batch size repeats
        for ln in [plain] + far:
            ln.inner_step(b)
        torch.cuda.synchronize()                          # (every learner steps on a stream of its own)
        for ln in far:
            assert memcheck.bits_equal(ln.last_loss, plain.last_loss)
    torch.cuda.synchronize()
    for ln in far:
        assert memcheck.bits_equal(ln.export_trainable(), plain.export_trainable()) and memcheck.bits_equal(ln.export_bn(), plain.export_bn())
        assert memcheck.bits_equal(ln.arena.grad, plain.arena.grad)
        rec, dropped = ln.read_clip_log()
        assert rec.shape[0] == 4 and dropped == 0 and not rec["flags"].any() and (rec["scale"] == 1.0).all() and float(rec["g_l2"].max()) > 0
        assert ln.read_clip_log()[0].shape[0] == 0
    for ln in [plain] + far:
        ln.close()


def _optimizer_reference(optimizer, L, theta0, grad):
    """What the fused optimizer op produces from copies of the initial state and `grad` (the launch Learner._apply issues)."""
    from mliis_amd import ops
    torch.cuda.synchronize()
    with torch.cuda.stream(L.stream):
        theta = theta0.clone()
        if optimizer == "sgd":
            ops.sgd_fused(theta, grad.clone(), L.lr, L.arena.l2_quad_mask, 0.0, L.lr_dev, l1=0.0)
        else:
            ops.adam_b1zero_fused(theta, grad.clone(), torch.zeros_like(theta), torch.zeros(1, dtype=torch.float32, device=theta.device), L.lr,
                                  L.arena.l2_quad_mask, 0.0, L.lr_dev, l1=0.0, ticket=torch.zeros(1, dtype=torch.int32, device=theta.device))
    torch.cuda.synchronize()
    return theta


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("mode", ["norm", "ratio"])
def test_a_clipped_step_consumes_the_twins_gradient_times_the_recorded_scale(optimizer, mode):
    twin = _twin(optimizer)
    if mode == "norm":
        clip = ("norm", 0.5 * twin["norm"])               # half the norm the unclipped twin reports for the same step
    else:                                                 # the median of ||g_t|| / max(||theta_t||, eps): about half the tensors clip
        clip = ("ratio", float(np.median([g / max(t, 1e-3) for g, t in twin["ratios"]])), 1e-3)
    L = _learner(optimizer, grad_clip=clip)
    L.load_task(*_task())
    torch.cuda.synchronize()
    assert memcheck.bits_equal(L.arena.theta, twin["theta0"])
    L.inner_step(BATCHES[0])
    torch.cuda.synchronize()
    rec, dropped = L.read_clip_log()
    assert rec.shape == (1, 1 if mode == "norm" else len(L.arena.trainable)) and dropped == 0 and not (rec["flags"] & BYPASSED).any()
    g0 = twin["grad"].cpu().numpy()
    scaled = g0.copy()
    if mode == "norm":
        _within_one_spacing(rec["g_l2"][0, 0], twin["norm"], "g_l2 against the twin's packed gradient")
        _within_one_spacing(rec["scale"][0, 0], float(np.float32(clip[1])) / twin["norm"], "scale")
        assert int(rec["flags"][0, 0]) == CLIPPED
        scaled = g0 * rec["scale"][0, 0]
    else:
        flags = rec["flags"][0]
        assert 0 < int((flags == CLIPPED).sum()) < len(flags) and ((rec["scale"][0] < 1.0) <= (flags == CLIPPED)).all()
        for t, p in enumerate(L.arena.trainable):
            o, gn, tn = L.arena.t_off[p.name], *twin["ratios"][t]
            _within_one_spacing(rec["g_l2"][0, t], gn, "tensor {} g_l2".format(t))
            if flags[t]:
                _within_one_spacing(rec["scale"][0, t], float(np.float32(clip[1])) * max(tn, float(np.float32(1e-3))) / gn, "tensor {} scale".format(t))
                scaled[o:o + (p.size + 3) // 4 * 4] = g0[o:o + (p.size + 3) // 4 * 4] * rec["scale"][0, t]
    assert scaled.dtype == np.float32
    got = L.arena.grad.cpu().numpy()
    assert got.tobytes() == scaled.tobytes()              # the twin's gradient times the recorded scale, one fp32 product per element
    want = _optimizer_reference(optimizer, L, twin["theta0"], torch.from_numpy(scaled).to(L.device))
    assert memcheck.bits_equal(L.arena.theta, want) and not memcheck.bits_equal(L.arena.theta, twin["theta1"])
    L.close()


def test_six_steps_replayed_from_a_graph_equal_six_eager_steps():
    twin = _twin("sgd")
    runs = []
    for use_graph in (True, False):
        L = _learner("sgd", grad_clip=("norm", 0.5 * twin["norm"]), use_graph=use_graph, clip_log=4)
        L.load_task(*_task())
        for b in (BATCHES[0], BATCHES[3]) * 3:
            L.inner_step(b)
        if use_graph:
            assert L.plans[2].graphs and L.plans[2].steps_run == 6
        rec, dropped = L.read_clip_log()                  # six rows into a ring of four: the two oldest are gone
        assert rec.shape == (4, 1) and dropped == 2 and (rec["flags"] & CLIPPED).any()
        torch.cuda.synchronize()
        runs.append((L.export_trainable(), rec.tobytes(), L._clip_ring.cpu().numpy().tobytes(), int(L._clip_cursor.item())))
        L.close()
    assert memcheck.bits_equal(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:] and runs[0][3] == 6


# ------------------------------------------------------------------------------------------------ the meta-learner
STEP = dict(num_shots=4, inner_batch_size=2, inner_iters=2, meta_step_size=0.5, meta_batch_size=2)


def _device_tasks(nan_in=()):
    from mliis_amd import metaseg
    tasks = []
    for i in range(2):
        x, y = metaseg.synthetic_task(4, H, seed=30 + i)
        if i in nan_in:
            x[0, 7, 9, 1] = np.nan                                # one pixel of the task's first image
        tasks.append(metaseg.DeviceTask("t%d" % i, torch.tensor(x, device="cuda"), torch.tensor(y, device="cuda")))
    return tasks


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


@pytest.mark.parametrize("mode", ["norm", "ratio"])
def test_a_meta_batch_on_a_lane_equals_task_by_task(mode):
    from mliis_amd.reptile import Gecko
    twin = _twin("sgd")
    clip = ("norm", 0.5 * twin["norm"]) if mode == "norm" else ("ratio", float(np.median([g / max(t, 1e-3) for g, t in twin["ratios"]])), 1e-3)
    tasks = _device_tasks()
    rows, thetas, records = [], [], []
    for n_lanes in (0, 1):
        L = _learner("sgd", step_log=64, grad_clip=clip)
        lanes = [_learner("sgd", seed=50, step_log=64, grad_clip=clip) for _ in range(n_lanes)]
        meta = _quiet(Gecko, L, rng_mode="per_task", seed=9, lanes=lanes, step_log=True)
        assert meta.clip_log
        _quiet(meta.train_step, tasks, **STEP)
        assert meta._lanes_in_use() == bool(n_lanes)
        rows.append(meta.inner_loop_summary)
        thetas.append(L.export_trainable())
        # the rows themselves, by task: task 0 ran on the main learner either way, task 1 on the lane when there is one
        per = [ln.read_clip_log()[0] for ln in [L] + lanes]
        records.append(np.concatenate(per).tobytes())
        for ln in [L] + lanes:
            ln.close()
    assert rows[0] == rows[1] and rows[0]["tasks"] == 2 and rows[0]["clip_frac"] > 0 and rows[0]["clip_bypassed"] == 0
    assert 0 < rows[0]["clip_scale_min"] < 1 and rows[0]["grad_l2_preclip_first"] > 0
    assert memcheck.bits_equal(thetas[0], thetas[1]) and records[0] == records[1] and len(records[0]) == 4 * 32 * (1 if mode == "norm" else 169)


def test_with_the_step_log_on_its_grad_l2_is_the_clipped_norm():
    twin = _twin("sgd")
    C = 0.5 * twin["norm"]
    L, plain = _learner("sgd", grad_clip=("norm", C), step_log=8), _learner("sgd", step_log=8)
    x, y = _task()
    for ln in (L, plain):
        ln.load_task(x, y)
        for b in BATCHES:
            ln.inner_step(b)
    steps, _ = L.read_step_log()
    clips, dropped = L.read_clip_log(last_read=True)
    own, _ = L.read_clip_log()                            # the clip's own cursor: the same four rows
    base, _ = plain.read_step_log()
    assert len(steps) == 4 and clips.shape == (4, 1) and dropped == 0 and own.tobytes() == clips.tobytes()
    C32 = float(np.float32(C))
    for k in range(4):
        print("step {}: pre-clip {!r}, scale {!r}, step log grad_l2 {!r}, bound {!r}".format(k, clips["g_l2"][k, 0], clips["scale"][k, 0],
                                                                                          steps["grad_l2"][k], C32))
        if clips["flags"][k, 0] & CLIPPED:                # one rounding of the scale, n of the products, the record's own
            assert float(steps["grad_l2"][k]) <= C32 * (1 + 2.0 ** -20)
        else:
            _within_one_spacing(steps["grad_l2"][k], float(clips["g_l2"][k, 0]), "an unclipped step's two norms")
    assert clips["flags"][0, 0] & CLIPPED
    # the first step starts from the same parameters in both learners: the pre-clip norm is the unclipped twin's step-log norm
    assert abs(float(clips["g_l2"][0, 0]) - float(base["grad_l2"][0])) <= float(np.spacing(base["grad_l2"][0]))
    for ln in (L, plain):
        ln.close()


def test_a_nan_pixel_bypasses_the_clip_and_the_guard_sees_what_it_always_saw():
    from mliis_amd import steplog as S
    from mliis_amd.reptile import Gecko
    x, y = _task()
    x = np.array(x, copy=True)
    x[0, 7, 9, 1] = np.nan
    pairs = {}
    for mode, clip in (("norm", ("norm", 1e-3)), ("ratio", ("ratio", 1e-4, 1e-3))):       # bounds any finite gradient would exceed
        L, plain = _learner("sgd", grad_clip=clip, step_log=8), _learner("sgd", step_log=8)
        for ln in (L, plain):
            ln.load_task(x, y)
            ln.inner_step([0, 1])
        steps, _ = L.read_step_log()
        clips, _ = L.read_clip_log(last_read=True)
        base, _ = plain.read_step_log()
        torch.cuda.synchronize()
        assert int(base["grad_nonfinite"][0]) > 0 and steps.tobytes() == base.tobytes()   # the step log's record is the one without clipping
        assert memcheck.bits_equal(L.arena.grad, plain.arena.grad) and memcheck.bits_equal(L.arena.theta, plain.arena.theta)
        assert (clips["flags"] == BYPASSED).all() and (clips["scale"] == 1.0).all()
        assert int(clips["nonfinite"][0].astype(np.uint64).sum()) == int(base["grad_nonfinite"][0])
        for ln in (L, plain):
            ln.close()
    tasks = _device_tasks(nan_in=(0, 1))
    L = _learner("sgd", seed=1, grad_clip=("norm", 1e-3), step_log=64)
    meta = _quiet(Gecko, L, rng_mode="per_task", seed=9, on_divergence="abort")
    with pytest.raises(S.DivergenceError), contextlib.redirect_stdout(io.StringIO()):
        meta.train_step(tasks, **dict(STEP, inner_batch_size=4))
    assert meta.inner_loop_summary["clip_bypassed"] >= 1 and meta.inner_loop_summary["nonfinite_steps"] >= 1
    L.close()


def test_without_grad_clip_nothing_is_loaded_allocated_or_launched():
    from mliis_amd import ops
    from mliis_amd._lib import MliisError, clip_lib, lib
    saved = clip_lib._dll
    clip_lib._dll = None                                  # as in a process that never touched the library
    try:
        L = _learner("sgd")
        assert L.grad_clip is None and L.clip_log == 0
        assert L._clip_table is None and L._clip_ws is None and L._clip_ring is None and L._clip_cursor is None and L._clip_pin is None
        L.load_task(*_task())
        lib.trace, clip_lib.trace, ops.PROFILE = [], [], []
        try:
            L.inner_step(BATCHES[0])                      # eager: the launch names of ops' timing hook as well
            launches, ops.PROFILE = [r["op"] for r in ops.PROFILE], None
            for b in (BATCHES[3], BATCHES[0]):            # captured, replayed
                L.inner_step(b)
            L.synchronize()
            names, clip_names = [n for n, _ in lib.trace], [n for n, _ in clip_lib.trace]
        finally:
            lib.trace, clip_lib.trace, ops.PROFILE = None, None, None
        assert names and not [n for n in names if n.startswith("mliis_clip")] and clip_names == [] and "clip_apply" not in launches
        assert clip_lib._dll is None                      # never loaded
        with pytest.raises(MliisError, match="grad_clip=None"):
            L.read_clip_log()
        with pytest.raises(ValueError):
            _learner("sgd", clip_log=8)
        # (clip.parse's other refusals: tests/test_clip_cpu.py.  This module builds 32 learners in all, each with a stream from torch's pool of
        # 32: one full turn, so the modules behind it find the pool where a suite without this file leaves it -- the co-residency that
        # tests/test_interference_gpu.py characterises depends on which pool streams its rig draws)
        for bad in (("norm", 0.0), ("both", 1.0)):
            with pytest.raises(ValueError):
                _learner("sgd", grad_clip=bad)
        L.close()
        # with it, the eager step issues exactly one call, between the backward pass and the optimizer launch
        on = _learner("sgd", grad_clip=("norm", 1.0))
        on.load_task(*_task())
        clip_lib.trace, ops.PROFILE = [], []
        try:
            on.inner_step(BATCHES[0])
            clip_names, with_clip = [n for n, _ in clip_lib.trace], [r["op"] for r in ops.PROFILE]
        finally:
            clip_lib.trace, ops.PROFILE = None, None
        assert clip_names == ["mliis_clip_apply"] and with_clip.count("clip_apply") == 1 and [n for n in with_clip if n != "clip_apply"] == launches
        on.close()
    finally:
        if clip_lib._dll is None:
            clip_lib._dll = saved
