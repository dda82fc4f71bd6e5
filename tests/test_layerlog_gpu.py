"""The inner loop's per-tensor log on the device: mliis_layerlog_append (csrc/layerlog.hip, libmliis_layerlog.so) through
ops.layerlog_append against numpy in float64 per tensor -- values, padding, determinism, the ring row and the cursor it only reads, the
memory contract, the delta mode, the argument errors -- then Learner(step_log=CAPACITY, layer_log=True) against what a host that
synchronises after every step reads and against the step log's own record, and Gecko(layer_log=True) over a lane, on a task with a NaN
pixel and with an interval."""
import contextlib
import ctypes as C
import io
import json
import os

import numpy as np
import pytest
import torch

import memcheck

pytestmark = pytest.mark.gpu

H = 64
SENTINEL = 0x5A5A5A5A
NONE = 0xFFFFFFFF


def _ch():
    from mliis_amd._lib import layerlog_lib
    return 4 * layerlog_lib.size("mliis_layerlog_chunk_quads")


def _sizes():
    CH = _ch()
    return [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, CH - 1, CH, CH + 1, 3 * CH + 7]


def _offsets(sizes):
    off, o = [], 0
    for s in sizes:
        off.append(o)
        o += (s + 3) // 4 * 4
    return off, o


def _planted(seed):
    """Two arenas of _sizes() tensors: N(0,1) everywhere, NaN in EVERY padding float, and per tensor (index in _sizes()):
    x: 5 (63) entirely non-finite; 6 (64) NaN at element 0; 7 (65) +inf at its last valid element; 8 (255) one 1e30; 9 (256) denormals;
       10 (257) all zero; 11 (CH - 1) -inf at its last valid element; 14 (3 CH + 7) NaNs in its third and fourth chunk.
    y: 2 (3) +inf at its last valid element; 5 entirely non-finite; 10 all zero; 12 (CH) NaN at element 0 and at its last;
       13 (CH + 1) NaN in its one-element second chunk; 14 a 1e30 and denormals."""
    sizes = _sizes()
    CH = _ch()
    off, n = _offsets(sizes)
    g = np.random.default_rng(seed)
    x, y = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    for a in (x, y):
        a[off[5]:off[5] + 63] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), 63)
        a[off[10]:off[10] + 257] = 0.0
    x[off[6]] = np.nan
    x[off[7] + 64] = np.inf
    x[off[8] + 100] = 1e30
    x[off[9] + 10:off[9] + 14] = np.array([1e-40, -2e-42, 1.4e-45, -5e-39], dtype=np.float32)
    x[off[11] + CH - 2] = -np.inf
    x[off[14] + 2 * CH + 5], x[off[14] + 2 * CH + 900], x[off[14] + 3 * CH + 6] = np.nan, np.inf, np.nan
    y[off[2] + 2] = np.inf
    y[off[12]], y[off[12] + CH - 1] = np.nan, np.nan
    y[off[13] + CH] = np.nan
    y[off[14] + 7], y[off[14] + CH + 1:off[14] + CH + 3] = 1e30, np.array([1e-41, -1e-44], dtype=np.float32)
    for t, s in enumerate(sizes):                       # a NaN parked in the padding must not show
        for a in (x, y):
            a[off[t] + s:off[t] + (s + 3) // 4 * 4] = np.nan
    return sizes, off, x, y


def _expected(sizes, off, x, y):
    """One record per tensor from float64 numpy: (l2 rounded once, absmax, non-finite count, first non-finite index) of x and of y."""
    out = np.zeros(len(sizes), dtype=[("x_l2", "<f4"), ("x_absmax", "<f4"), ("y_l2", "<f4"), ("y_absmax", "<f4"), ("x_nonfinite", "<u4"),
                                      ("y_nonfinite", "<u4"), ("x_first", "<u4"), ("y_first", "<u4")])
    for t, s in enumerate(sizes):
        for k, a in (("x", x), ("y", y)):
            v = a[off[t]:off[t] + s]
            fin = np.isfinite(v)
            v64 = v[fin].astype(np.float64)
            out[k + "_l2"][t] = np.float32(np.sqrt(np.sum(v64 * v64)))
            out[k + "_absmax"][t] = np.abs(v[fin]).max() if fin.any() else 0.0
            out[k + "_nonfinite"][t] = int((~fin).sum())
            out[k + "_first"][t] = int(np.flatnonzero(~fin)[0]) if (~fin).any() else NONE
    return out


def _assert_records(got, want, what=""):
    """Words 0 and 2 within one fp32 ulp of the float64 result rounded once (the order of the double summation is the only freedom);
    every other word bit for bit."""
    assert got.shape == want.shape
    for t in range(len(want)):
        for k in ("x_l2", "y_l2"):
            print("{} tensor {} {}: device {!r}, float64 numpy rounded to f32 {!r}".format(what, t, k, got[k][t], want[k][t]))
            assert abs(float(got[k][t]) - float(want[k][t])) <= float(np.spacing(want[k][t])), (what, t, k)
        for k in ("x_absmax", "y_absmax", "x_nonfinite", "y_nonfinite", "x_first", "y_first"):
            assert got[k][t].tobytes() == want[k][t].tobytes(), (what, t, k, got[k][t], want[k][t])


def _ring(capacity, T):
    ring = memcheck.guarded_buffer(capacity * T * 8, fill=0.0).view(torch.int32).view(capacity, T, 8)
    ring.fill_(SENTINEL)
    return ring


def _cursor(value):
    c = memcheck.guarded_buffer(1, fill=0.0).view(torch.int32)
    c.fill_(value - (1 << 32) if value >= (1 << 31) else value)
    return c


def _host(ring):
    from mliis_amd import layerlog as LL
    torch.cuda.synchronize()
    return ring.cpu().numpy().view(LL.RECORD_DTYPE).reshape(ring.shape[0], ring.shape[1])


def test_records_against_float64_numpy_with_ring_cursor_padding_and_guards():
    from mliis_amd import ops
    sizes, off, x_h, y_h = _planted(seed=3)
    want = _expected(sizes, off, x_h, y_h)
    T = len(sizes)
    # the plants are where the docstring says: counts and first indices by hand
    CH = _ch()
    assert want["x_nonfinite"].tolist() == [0, 0, 0, 0, 0, 63, 1, 1, 0, 0, 0, 1, 0, 0, 3]
    assert want["x_first"].tolist() == [NONE] * 5 + [0, 0, 64, NONE, NONE, NONE, CH - 2, NONE, NONE, 2 * CH + 5]
    assert want["y_nonfinite"].tolist() == [0, 0, 1, 0, 0, 63, 0, 0, 0, 0, 0, 0, 2, 1, 0]
    assert want["y_first"].tolist() == [NONE, NONE, 2, NONE, NONE, 0] + [NONE] * 6 + [0, CH, NONE]
    assert want["x_l2"][5] == 0 and want["x_absmax"][5] == 0 and want["x_l2"][10] == 0 and want["x_absmax"][8] == np.float32(1e30)
    memcheck.reset_guards()
    x, y = memcheck.guarded_input(torch.from_numpy(x_h)), memcheck.guarded_input(torch.from_numpy(y_h))
    table = ops.layerlog_table(sizes, x.device)
    assert table.T == T and table.n == x.numel() and table.nchunks == T + 1 + 3
    ws = memcheck.guarded_buffer(ops.layerlog_workspace(table).numel(), fill=0.0).view(torch.int32)
    ws.fill_(SENTINEL)                                   # (its contents before a launch do not matter)
    snap = memcheck.snapshot(x, y)
    # cursor 0, capacity - 1 and 2^32 - 1, each with row_offset 1: rows 1, 0 (wrapped by the ring) and 0 (wrapped by the counter)
    for capacity, cur, row in ((4, 0, 1), (4, 3, 0), (3, (1 << 32) - 1, 0)):
        ring, cursor = _ring(capacity, T), _cursor(cur)
        assert ops.layerlog_append(x, y, table, ws, cursor, out=ring, row_offset=1) is ring
        r = _host(ring)
        _assert_records(r[row], want, "cursor %d" % cur)
        others = [k for k in range(capacity) if k != row]
        assert bool((ring[others] == SENTINEL).all()) and (int(cursor.item()) & 0xFFFFFFFF) == cur          # one row; the cursor is only read
    # no cursor counts as 0; the same inputs give the same bits, launch after launch and row after row
    ring = _ring(4, T)
    ops.layerlog_append(x, y, table, ws, None, out=ring, row_offset=2)
    first = _host(ring)[2].tobytes()
    ops.layerlog_append(x, y, table, ws, None, out=ring, row_offset=2)
    ops.layerlog_append(x, y, table, ws, None, out=ring, row_offset=7)
    r = _host(ring)
    assert r[2].tobytes() == first == r[3].tobytes() and bool((ring[:2] == SENTINEL).all())
    _assert_records(r[2], want, "no cursor")
    snap.assert_unchanged()
    memcheck.assert_guards()


def test_delta_mode_is_the_fp32_difference_reduced_in_float64():
    from mliis_amd import ops
    sizes, off, a_h, b_h = _planted(seed=8)
    with np.errstate(invalid="ignore"):
        d_h = a_h - b_h                                  # one fp32 subtraction per element (inf - inf and NaN - x: NaN)
    assert d_h.dtype == np.float32
    want = _expected(sizes, off, d_h, b_h)
    memcheck.reset_guards()
    a, b = memcheck.guarded_input(torch.from_numpy(a_h)), memcheck.guarded_input(torch.from_numpy(b_h))
    table = ops.layerlog_table(sizes, a.device)
    ws = memcheck.guarded_buffer(ops.layerlog_workspace(table).numel(), fill=0.0).view(torch.int32)
    ring = _ring(2, len(sizes))
    snap = memcheck.snapshot(a, b)
    ops.layerlog_append(a, b, table, ws, None, out=ring, row_offset=1, mode="delta")
    r = _host(ring)
    _assert_records(r[1], want, "delta")
    assert bool((ring[0] == SENTINEL).all())
    # a buffer against itself: every finite element gives 0, every non-finite one NaN
    ops.layerlog_append(a, a, table, ws, None, out=ring, row_offset=0, mode="delta")
    r = _host(ring)
    same = _expected(sizes, off, a_h, a_h)
    assert r["x_l2"][0].tolist() == [0.0] * len(sizes) and r["x_absmax"][0].tolist() == [0.0] * len(sizes)
    assert r["x_nonfinite"][0].tolist() == same["x_nonfinite"].tolist() and r["x_first"][0].tolist() == same["x_first"].tolist()
    snap.assert_unchanged()
    memcheck.assert_guards()


def test_bad_arguments_are_refused_before_any_launch():
    from mliis_amd import layerlog as LL
    from mliis_amd import ops
    from mliis_amd._lib import MliisError, layerlog_lib
    sizes = [5, 300, 64]
    _, n = _offsets(sizes)
    memcheck.reset_guards()
    x, y = torch.randn(n + 4, device="cuda"), torch.randn(n + 4, device="cuda")
    table = ops.layerlog_table(sizes, x.device)
    T, nch = table.T, table.nchunks
    ring, cursor = _ring(2, T), _cursor(0)
    need = layerlog_lib.size("mliis_layerlog_workspace_bytes", nch)
    ws = memcheck.guarded_buffer(need // 4 + 4, fill=0.0).view(torch.int32)
    ws.fill_(SENTINEL)
    raw = layerlog_lib.load().mliis_layerlog_append
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)   # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    good = [0, p(x), p(y), n, p(table.chunks), nch, p(table.segs), T, p(ws), need, p(ring), 2, p(cursor), 0, st]
    ARG, ALIGN = -1, -3
    cases = []
    for i in (1, 2, 4, 6, 8, 10):                        # every pointer but the cursor null in turn
        cases.append((ARG, good[:i] + [None] + good[i + 1:]))
    for mode in (-1, 2):
        cases.append((ARG, [mode] + good[1:]))
    for bad_n in (0, -4, n + 2, 3):
        cases.append((ARG, good[:3] + [bad_n] + good[4:]))
    for bad_t in (0, -1, nch + 1):                       # no tensor; more tensors than chunks
        cases.append((ARG, good[:7] + [bad_t] + good[8:]))
    for bad_c in (0, T - 1, n // 4 + 1):                 # fewer chunks than tensors; more chunks than quads
        cases.append((ARG, good[:5] + [bad_c] + good[6:]))
    for cap in (0, -1):
        cases.append((ARG, good[:11] + [cap] + good[12:]))
    cases.append((ARG, good[:9] + [need - 1] + good[10:]))          # a workspace one byte short
    for i, t in ((1, x), (2, y), (4, table.chunks), (6, table.segs), (8, ws), (10, ring)):
        cases.append((ALIGN, good[:i] + [p(t, 4)] + good[i + 1:]))
    cases.append((ALIGN, good[:12] + [p(cursor, 2)] + good[13:]))
    for code, args in cases:
        assert raw(*args) == code, args
        assert layerlog_lib.load().mliis_layerlog_last_error().startswith(b"layerlog_append:")
    torch.cuda.synchronize()
    assert bool((ring == SENTINEL).all()) and bool((ws == SENTINEL).all()) and int(cursor.item()) == 0       # nothing ran
    # the wrapper: tensors of the wrong kind, size or place, a wrong out=, a table that is none
    ok = dict(x=x[:n], y=y[:n], table=table, ws=ws, cursor=cursor, out=ring)
    wide = torch.zeros(2, T, 16, dtype=torch.int32, device="cuda")
    for change in (dict(x=x[:n - 4]), dict(y=y[:n + 4]), dict(x=x[::2][:n // 2], y=y[:n // 2]), dict(x=x[:n].double()), dict(x=x[:n].cpu()),
                   dict(table=(table.chunks, table.segs)), dict(ws=ws[:need // 4 - 1]), dict(ws=ws.to(torch.int64)), dict(ws=ws.cpu()),
                   dict(cursor=torch.zeros(2, dtype=torch.int32, device="cuda")), dict(cursor=torch.zeros(1, device="cuda")),
                   dict(out=wide[:, :, :8]), dict(out=torch.zeros(2, T + 1, 8, dtype=torch.int32, device="cuda")),
                   dict(out=torch.zeros(2, T, 8, dtype=torch.float32, device="cuda")), dict(out=torch.zeros(2, T, 8, dtype=torch.int32)),
                   dict(out=torch.zeros(2 * T, 8, dtype=torch.int32, device="cuda")), dict(out=ring, capacity=3), dict(out=None),
                   dict(out=None, capacity=0), dict(mode="both"), dict(row_offset=-1), dict(row_offset=1 << 32)):
        with pytest.raises(MliisError):
            ops.layerlog_append(**dict(ok, **change))
    # tables are validated on the host before they are uploaded
    t = LL.chunk_table(sizes, _ch() // 4)
    for chunks, segs, nn in ((t.chunks, t.segs, t.n - 4), (t.chunks[:-1], t.segs, t.n), (t.chunks, t.segs[::-1].copy(), t.n)):
        with pytest.raises(MliisError, match="layerlog_table"):
            ops.layerlog_table(None, x.device, chunks=chunks, segs=segs, n=nn)
    with pytest.raises(MliisError):
        ops.layerlog_table(sizes, "cpu")
    torch.cuda.synchronize()
    assert bool((ring == SENTINEL).all()) and bool((ws == SENTINEL).all())
    fresh = ops.layerlog_append(x[:n], y[:n], table, ws, cursor, capacity=3)     # and the form that allocates the ring
    assert tuple(fresh.shape) == (3, T, 8) and fresh.dtype == torch.int32 and bool(fresh[0].any()) and not bool(fresh[1:].any())
    memcheck.assert_guards()


# ------------------------------------------------------------------------------------------------ the learner
BATCHES = [[0, 1], [2, 3], [1, 2], [3, 0]]


def _host_rows(L):
    """What a host that synchronises reads off the arenas, per tensor in float64: (grad l2, grad absmax, theta l2, theta absmax)."""
    L.synchronize()
    out = []
    for name in L.layer_log_names:
        g, w = L.arena.g[name].cpu().numpy().reshape(-1), L.arena.w[name].cpu().numpy().reshape(-1)
        assert np.isfinite(g).all() and np.isfinite(w).all()
        out.append((np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2))), np.abs(g).max(), np.float32(np.sqrt(np.sum(w.astype(np.float64) ** 2))),
                    np.abs(w).max()))
    return out


@pytest.mark.parametrize("optimizer,precision", [("sgd", "fp32"), ("adam", "bf16")])
def test_learner_rows_equal_a_synchronising_host_and_the_step_log(optimizer, precision):
    from mliis_amd import layerlog as LL
    from mliis_amd import metaseg, ops
    from mliis_amd._lib import MliisError, layerlog_lib
    from mliis_amd.learner import Learner
    kw = dict(image_size=H, rsd=[2, 4], drop_connect=False, optimizer=optimizer, matmul_precision=precision, seed=5, use_graph=True,
              learning_rate=1e-3)
    L, L0, Lp = Learner(step_log=8, layer_log=True, **kw), Learner(step_log=8, layer_log=False, **kw), Learner(step_log=8, **kw)
    T = len(L.layer_log_names)
    assert L.layer_log_names == [p.name for p in L.arena.trainable] and tuple(L._layer_ring.shape) == (8, T, 8) == tuple(L._delta_ring.shape)
    for off in (L0, Lp):                                  # off: nothing is allocated
        assert off.layer_log is False and off._layer_ring is None and off._layer_table is None and off._layer_ws is None and off._delta_ring is None
    with pytest.raises(ValueError, match="step_log"):
        Learner(layer_log=True, **kw)
    x, y = metaseg.synthetic_task(4, H, seed=11)
    for ln in (L, L0, Lp):
        ln.load_task(x, y)
    seen, names = [], {}
    for k, b in enumerate(BATCHES):
        for ln in (L, L0, Lp):
            if k == 0:                                    # the eager step: the launch names of ops' timing hook, the library's own calls
                ops.PROFILE, layerlog_lib.trace = [], []
            try:
                ln.inner_step(b)
                if k == 0:
                    names[id(ln)] = ([r["op"] for r in ops.PROFILE], [name for name, _ in layerlog_lib.trace])
            finally:
                ops.PROFILE, layerlog_lib.trace = None, None
        seen.append(_host_rows(L))                        # what a host without the log would have to do after every step
    # with layer_log off the launch sequence is that of a learner built without the argument; on, one call in front of the step log's
    assert names[id(L0)] == names[id(Lp)] and names[id(L0)][1] == [] and "layerlog_append" not in names[id(L0)][0]
    on = names[id(L)][0]
    assert on.count("layerlog_append") == 1 and on[on.index("layerlog_append") + 1] == "steplog_append" and on[-1] == "steplog_append"
    assert [n for n in on if n != "layerlog_append"] == names[id(L0)][0] and names[id(L)][1] == ["mliis_layerlog_append"]
    assert L.plans[2].graphs and L.plans[2].steps_run == 4        # steps 3 and 4 were replays of one captured graph
    rows, dropped = L.read_layer_log()
    assert rows.dtype == LL.RECORD_DTYPE and rows.shape == (4, T) and dropped == 0
    again, _ = L.read_layer_log()                          # reading consumes nothing ...
    assert again.tobytes() == rows.tobytes()
    for k, host in enumerate(seen):
        for t, (gl2, gmax, wl2, wmax) in enumerate(host):
            assert abs(float(rows["x_l2"][k, t]) - float(gl2)) <= float(np.spacing(gl2)), (k, t)
            assert abs(float(rows["y_l2"][k, t]) - float(wl2)) <= float(np.spacing(wl2)), (k, t)
            assert rows["x_absmax"][k, t].tobytes() == np.float32(gmax).tobytes() and rows["y_absmax"][k, t].tobytes() == np.float32(wmax).tobytes()
    assert not rows["x_nonfinite"].any() and not rows["y_nonfinite"].any()
    assert (rows["x_first"] == NONE).all() and (rows["y_first"] == NONE).all()
    assert len({rows["x_l2"][k].tobytes() for k in range(4)}) == 4 and float(rows["x_l2"].max()) > 0        # four different steps
    # against the step log's record of the same steps
    rec, dropped = L.read_step_log()                       # ... not of the step log either
    assert len(rec) == 4 and dropped == 0
    for k in range(4):
        assert int(rows["x_nonfinite"][k].astype(np.uint64).sum()) == int(rec["grad_nonfinite"][k])
        assert rows["x_absmax"][k].max().tobytes() == rec["grad_absmax"][k].tobytes()
        total = np.float32(np.sqrt(np.sum(rows["x_l2"][k].astype(np.float64) ** 2)))
        print("step {} sqrt(sum grad_l2^2) {!r}, step log grad_l2 {!r}".format(k, total, rec["grad_l2"][k]))
        assert abs(float(total) - float(rec["grad_l2"][k])) <= 4 * float(np.spacing(rec["grad_l2"][k]))
    # the shared "seen" cursor has moved: nothing new -- but the rows of the steps that read returned are still there
    assert L.read_layer_log()[0].shape == (0, T)
    last, dropped = L.read_layer_log(last_read=True)
    assert last.tobytes() == rows.tobytes() and dropped == 0
    # training is unchanged: loss and parameters bit for bit those of the learner without the log
    assert memcheck.bits_equal(L.last_loss, L0.last_loss) and memcheck.bits_equal(L.export_trainable(), L0.export_trainable())
    assert memcheck.bits_equal(L.export_bn(), L0.export_bn()) and memcheck.bits_equal(Lp.export_trainable(), L0.export_trainable())
    with pytest.raises(MliisError, match="layer_log=False"):
        L0.read_layer_log()
    # layer_delta: ||a - b|| per tensor against the fp32 difference reduced in float64 on the host
    a, b = L.export_trainable(), Lp.export_trainable().clone()
    b.mul_(0.5)
    L.layer_delta(a, b, row=3)
    d = L.read_layer_deltas([3, 0])
    assert d.shape == (2, T) and not d[1].tobytes().strip(b"\0")
    diff, b_h = (a - b).cpu().numpy(), b.cpu().numpy()
    for t, p in enumerate(L.arena.trainable):
        o = L.arena.t_off[p.name]
        for field, v in (("x_l2", diff[o:o + p.size]), ("y_l2", b_h[o:o + p.size])):
            want = np.float32(np.sqrt(np.sum(v.astype(np.float64) ** 2)))
            assert abs(float(d[field][0, t]) - float(want)) <= float(np.spacing(want)), (t, field)
    with pytest.raises(ValueError):
        L.layer_delta(a, b, row=8)
    for ln in (L, L0, Lp):
        ln.close()


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


def _learner(seed=1, layer_log=True, use_graph=True):
    from mliis_amd.learner import Learner
    return Learner(image_size=H, rsd=[2, 4], drop_connect=False, optimizer="sgd", seed=seed, use_graph=use_graph, learning_rate=5e-3, step_log=64,
                   layer_log=layer_log)


def _replay(E, tasks, seed, meta_iter, t, steps=None):
    """Task t of a meta-iteration stepped on learner E as Gecko steps it (the draws of Gecko._sample and _batches, replayed); stops after
    `steps` steps when given.  Returns the batches."""
    from mliis_amd import metaseg
    from mliis_amd.reptile import _task_rng
    rng = _task_rng(seed, meta_iter, t)
    images, labels = metaseg.sample_task(tasks, 4, rng)
    batches = [list(b) for b in metaseg.mini_batch_indices(4, 2, 2, False, rng)]
    E.load_task(images, labels)
    for b in batches[:steps]:
        E.inner_step(b)
    return batches


def test_row_over_a_lane_equals_task_by_task_and_delta_equals_the_host():
    from mliis_amd import layerlog as LL
    from mliis_amd.reptile import Gecko
    tasks = _device_tasks()
    rows, thetas = [], []
    for n_lanes in (0, 1):
        L, lanes = _learner(), [_learner(seed=50) for _ in range(n_lanes)]
        meta = _quiet(Gecko, L, rng_mode="per_task", seed=9, lanes=lanes, step_log=True, layer_log=True, layer_log_interval=1)
        old = L.export_trainable()
        _quiet(meta.train_step, tasks, **STEP)
        assert meta._lanes_in_use() == bool(n_lanes)
        rows.append(meta.inner_loop_layers_summary)
        thetas.append(L.export_trainable())
        for ln in lanes:
            ln.close()
    T = len(L.layer_log_names)
    assert rows[0] == rows[1] and rows[0]["tasks"] == 2 and rows[0]["meta_iter"] == 0 and rows[0]["first_nonfinite"] is None
    assert all(len(rows[0][k]) == T for k in ("grad_l2_first", "grad_l2_last", "grad_to_weight_last", "grad_absmax", "delta_l2", "delta_rel"))
    assert min(rows[0]["grad_l2_first"]) >= 0 and max(rows[0]["grad_l2_first"]) > 0 and max(rows[0]["delta_l2"]) > 0
    assert memcheck.bits_equal(thetas[0], thetas[1])
    json.dumps({k: LL._json_value(v) for k, v in rows[0].items()})
    # delta_l2: the mean over the two tasks of ||theta_task - old|| per tensor; the host takes the fp32 difference and reduces in float64
    E = _learner(layer_log=False)
    host = []
    for t in (0, 1):
        E.import_trainable(old)
        _replay(E, tasks, 9, 0, t)
        d = (E.export_trainable() - old).cpu().numpy()
        host.append([np.float32(np.sqrt(np.sum(d[E.arena.t_off[p.name]:E.arena.t_off[p.name] + p.size].astype(np.float64) ** 2)))
                     for p in E.arena.trainable])
    for t in range(T):       # each task's value within one ulp of the host's, so their mean within the mean of the two ulps
        want = (float(host[0][t]) + float(host[1][t])) / 2
        assert abs(rows[0]["delta_l2"][t] - want) <= (float(np.spacing(host[0][t])) + float(np.spacing(host[1][t]))) / 2, (t, rows[0]["delta_l2"][t], want)
    for ln in (L, E):
        ln.close()


def test_abort_on_a_nan_pixel_names_the_tensors_an_eager_host_sees():
    """One NaN pixel in the first image of a task: the forward pass carries it into the loss and every gradient it reaches."""
    from mliis_amd import steplog as S
    from mliis_amd.reptile import Gecko, _task_rng
    tasks = _device_tasks(nan_in=(1,))
    seed = next(s for s in range(200) if [_task_rng(s, 0, t).sample(list(tasks), 1)[0].name for t in (0, 1)] == ["t0", "t1"])
    L = _learner()
    theta0, bn0 = L.export_trainable(), L.export_bn()
    # the eager twin: task 1 stepped until the first batch that holds shot 0, looked at on the host after every step
    E = _learner(layer_log=False, use_graph=False)
    batches = _replay(E, tasks, seed, 0, 1, steps=0)
    first = next(j for j, b in enumerate(batches) if 0 in b)
    largest = None
    names = L.layer_log_names
    for j in range(first + 1):
        E.inner_step(batches[j])
        E.synchronize()
        g = {n: E.arena.g[n].cpu().numpy() for n in names}
        w = {n: E.arena.w[n].cpu().numpy() for n in names}
        if j == first - 1:
            amax = [float(np.abs(g[n]).max()) for n in names]
            largest = [(names[i], amax[i]) for i in sorted(range(len(names)), key=lambda i: (-amax[i], i))[:3]]
    bad_g = [n for n in names if not np.isfinite(g[n]).all()]
    bad_w = [n for n in names if not np.isfinite(w[n]).all()]
    assert bad_g                                                                   # the NaN did reach gradients
    meta = _quiet(Gecko, L, rng_mode="per_task", seed=seed, on_divergence="abort", layer_log=True, layer_log_interval=100)
    with pytest.raises(S.DivergenceError, match="task 1 step {}".format(first)) as ei, contextlib.redirect_stdout(io.StringIO()):
        meta.train_step(tasks, **STEP)
    e = ei.value
    assert e.grad_nonfinite == (len(bad_g), bad_g[:8]) and e.theta_nonfinite == (len(bad_w), bad_w[:8])
    assert e.largest_grads == largest and (largest is None) == (first == 0)
    assert bad_g[0] in str(e) and meta.meta_iter == 0
    assert meta.inner_loop_layers_summary["first_nonfinite"]["task"] == 1 and meta.inner_loop_layers_summary["first_nonfinite"]["step"] == first
    assert memcheck.bits_equal(L.export_trainable(), theta0) and memcheck.bits_equal(L.export_bn(), bn0)
    for ln in (L, E):
        ln.close()


def test_interval_two_writes_lines_for_iterations_0_and_2(tmp_path):
    from mliis_amd import layerlog as LL
    from mliis_amd.reptile import Gecko
    tasks = _device_tasks()
    L = _learner()
    meta = _quiet(Gecko, L, rng_mode="per_task", seed=9, step_log=True, layer_log=True, layer_log_interval=2)
    meta.inner_loop_layers_sink = LL.LayerLogWriter(str(tmp_path), L.layer_log_names).add
    for _ in range(3):
        _quiet(meta.train_step, tasks, **STEP)
    lines = [json.loads(ln) for ln in open(os.path.join(str(tmp_path), "inner_loop_layers.jsonl"))]
    assert [r["meta_iter"] for r in lines] == [0, 2] and all(r["tasks"] == 2 and r["first_nonfinite"] is None for r in lines)
    assert json.load(open(os.path.join(str(tmp_path), "inner_loop_layers.names.json"))) == L.layer_log_names
    assert lines[0]["grad_l2_first"] != lines[1]["grad_l2_first"] and len(lines[0]["delta_rel"]) == len(L.layer_log_names)
    L.close()
