"""The inner loop's step log on the device: mliis_steplog_append (csrc/steplog.hip, libmliis_steplog.so) through ops.steplog_append against
numpy in float64 -- values, determinism, the ring and its device cursor, the memory contract, the argument errors -- then
Learner(step_log=CAPACITY) against what a host that synchronises after every step reads (graph replays included), and
Gecko(step_log=True, on_divergence=...) over a lane and on a task with a NaN pixel."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest
import torch

import memcheck

pytestmark = pytest.mark.gpu

H = 64
# one quad; a few threads of one workgroup; one full grid of quads (256 x 256 threads) plus one quad; sixteen passes of the grid plus one
SIZES = [4, 1028, 262148, 1048580]


def _planted(n, seed, big):
    """N(0,1) gradient and parameters with the values a reduction can trip over: a NaN at 0, +inf at n - 1, -inf in the middle, one 1e30
    (its square overflows fp32, not the double sum; big=False leaves it out so that the N(0,1) part decides the norm), a few denormals;
    theta gets the same kinds in other numbers (n = 4 has room for the first two only)."""
    g = np.random.default_rng(seed)
    grad, theta = g.standard_normal(n).astype(np.float32), g.standard_normal(n).astype(np.float32)
    grad[0], grad[n - 1], grad[n // 2] = np.nan, np.inf, -np.inf
    if big:
        grad[1] = 1e30
    theta[0], theta[n - 1] = np.nan, np.inf
    if n >= 64:
        grad[10:14] = np.array([1e-40, -2e-42, 1.4e-45, -5e-39], dtype=np.float32)
        theta[n // 2], theta[20], theta[21], theta[3] = -np.inf, np.nan, np.nan, 1e30
        theta[30:32] = np.array([1e-41, -1e-44], dtype=np.float32)
    return grad, theta


def _expected(grad, theta):
    fin = np.isfinite(grad)
    g64 = grad[fin].astype(np.float64)
    l2 = np.float32(np.sqrt(np.sum(g64 * g64)))                 # float64 over the finite elements, rounded once
    amax = np.float32(np.abs(grad[fin]).max()) if fin.any() else np.float32(0)
    return l2, amax, int((~fin).sum()), int((~np.isfinite(theta)).sum())


def _log_buffers(capacity):
    """Ring, workspace and cursor, each zeroed and followed by a guard band."""
    from mliis_amd._lib import steplog_lib
    ring = memcheck.guarded_buffer(capacity * 8, fill=0.0).view(torch.int32).view(capacity, 8)
    ws = memcheck.guarded_buffer(steplog_lib.size("mliis_steplog_workspace_bytes") // 4, fill=0.0).view(torch.int32)
    cursor = memcheck.guarded_buffer(1, fill=0.0).view(torch.int32)
    return ring, ws, cursor


def _rows(ring):
    from mliis_amd import steplog as S
    torch.cuda.synchronize()
    return ring.cpu().numpy().view(S.RECORD_DTYPE).reshape(-1)


@pytest.mark.parametrize("big", [True, False], ids=["with-1e30", "normal-only"])
@pytest.mark.parametrize("n", SIZES)
def test_append_against_float64_numpy_with_ring_cursor_and_guards(n, big):
    from mliis_amd import ops
    grad_h, theta_h = _planted(n, seed=n + int(big), big=big)
    l2, amax, gnf, tnf = _expected(grad_h, theta_h)
    assert gnf == 3 and tnf == (5 if n >= 64 else 2) and (amax == np.float32(1e30)) == big
    memcheck.reset_guards()
    grad, theta = memcheck.guarded_input(torch.from_numpy(grad_h)), memcheck.guarded_input(torch.from_numpy(theta_h))
    loss_h = np.array([0.7, 0.6, 0.3, 123.0], dtype=np.float32)
    loss4, lr = memcheck.guarded_input(torch.from_numpy(loss_h)), memcheck.guarded_input(torch.tensor([2.5e-3]))
    ring, ws, cursor = _log_buffers(4)
    ring2, ws2, cursor2 = _log_buffers(2)
    snap = memcheck.snapshot(grad, theta, lr)
    for k in range(3):       # the third call sees another loss: the slots can be told apart
        if k == 2:
            loss4[0] = 9.5
        assert ops.steplog_append(loss4, lr, grad, theta, ws, cursor, out=ring) is ring
        ops.steplog_append(loss4, lr, grad, theta, ws2, cursor2, out=ring2)
    r, r2 = _rows(ring), _rows(ring2)
    print("n = {} grad_l2: device {!r}, float64 numpy rounded to f32 {!r}, ulp {:.3e}".format(n, r["grad_l2"][0], l2, float(np.spacing(l2))))
    # values: exact but for the norm, which may differ by the order of a double summation before its one rounding
    assert abs(float(r["grad_l2"][0]) - float(l2)) <= float(np.spacing(l2))
    assert r["grad_absmax"][0].tobytes() == amax.tobytes() and int(r["grad_nonfinite"][0]) == gnf and int(r["theta_nonfinite"][0]) == tnf
    assert r["loss"][0].tobytes() == loss_h[0].tobytes() and r["ce"][0].tobytes() == loss_h[1].tobytes()
    assert r["iou"][0].tobytes() == loss_h[2].tobytes() and r["lr"][0].tobytes() == np.float32(2.5e-3).tobytes()
    # the same inputs give the same bits; the third call landed in slot 2 (capacity 4) and in slot 0 (capacity 2)
    assert r[0].tobytes() == r[1].tobytes()
    assert r["loss"][2] == np.float32(9.5) and r[2].tobytes()[4:] == r[0].tobytes()[4:] and r[3].tobytes() == bytes(32)
    assert int(cursor.item()) == 3 and int(cursor2.item()) == 3
    assert r2[0].tobytes() == r[2].tobytes() and r2[1].tobytes() == r[1].tobytes()
    # the arrival counter is left at zero, the inputs untouched, nothing outside ring / workspace / cursor written
    assert int(ws[0].item()) == 0 and int(ws2[0].item()) == 0
    snap.assert_unchanged()
    memcheck.assert_guards()


def test_bad_arguments_are_refused_before_any_launch():
    from mliis_amd import ops
    from mliis_amd._lib import MliisError, steplog_lib
    n = 1028
    grad, theta = torch.randn(n + 4, device="cuda"), torch.randn(n + 4, device="cuda")
    loss4, lr = torch.ones(4, device="cuda"), torch.ones(1, device="cuda")
    ring, ws, cursor = _log_buffers(2)
    raw = steplog_lib.load().mliis_steplog_append
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)   # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    good = [p(loss4), p(lr), p(grad), p(theta), n, p(ws), p(ring), 2, p(cursor), st]
    ARG, ALIGN = -1, -3
    cases = []
    for i in (0, 1, 2, 3, 5, 6, 8):                       # every pointer null in turn
        cases.append((ARG, good[:i] + [None] + good[i + 1:]))
    for bad_n in (0, -4, 1026, 3):
        cases.append((ARG, good[:4] + [bad_n] + good[5:]))
    for cap in (0, -1):
        cases.append((ARG, good[:7] + [cap] + good[8:]))
    for i, t in ((2, grad), (3, theta), (5, ws), (6, ring)):   # 16-byte alignment of the arenas, the workspace and the ring
        cases.append((ALIGN, good[:i] + [p(t, 4)] + good[i + 1:]))
    for i, t in ((0, loss4), (1, lr), (8, cursor)):            # 4-byte alignment of the scalars
        cases.append((ALIGN, good[:i] + [p(t, 2)] + good[i + 1:]))
    for code, args in cases:
        assert raw(*args) == code, args
        assert steplog_lib.load().mliis_steplog_last_error().startswith(b"steplog_append:")
    torch.cuda.synchronize()
    assert int(cursor.item()) == 0 and not bool(ring.any()) and not bool(ws.any())       # nothing ran
    # the wrapper: views that would be read as dense, a wrong out=, tensors of the wrong kind
    ok = dict(loss4=loss4, lr_dev=lr, grad=grad[:n], theta=theta[:n], ws=ws, cursor=cursor, out=ring)
    wide = torch.zeros(2, 16, dtype=torch.int32, device="cuda")
    for change in (dict(grad=grad[::2][:n // 2], theta=theta[:n // 2]), dict(theta=theta[::2][:n // 2], grad=grad[:n // 2]),
                   dict(out=wide[:, :8]), dict(out=torch.zeros(2, 7, dtype=torch.int32, device="cuda")),
                   dict(out=torch.zeros(2, 8, dtype=torch.float32, device="cuda")), dict(out=torch.zeros(16, dtype=torch.int32, device="cuda")),
                   dict(out=torch.zeros(2, 8, dtype=torch.int32)), dict(out=ring, capacity=3), dict(out=None), dict(out=None, capacity=0),
                   dict(theta=theta[:n - 4]), dict(grad=grad[:n].double(), theta=theta[:n].double()), dict(grad=grad[:n].cpu()),
                   dict(ws=ws[:-1]), dict(ws=ws.to(torch.int64)), dict(cursor=torch.zeros(2, dtype=torch.int32, device="cuda")),
                   dict(cursor=torch.zeros(1, device="cuda")), dict(loss4=loss4[:2]), dict(loss4=torch.ones(8, device="cuda")[::2])):
        with pytest.raises(MliisError):
            ops.steplog_append(**dict(ok, **change))
    with pytest.raises(MliisError, match="multiple of 4"):
        ops.steplog_append(**dict(ok, grad=grad[:n + 2], theta=theta[:n + 2]))
    torch.cuda.synchronize()
    assert int(cursor.item()) == 0 and not bool(ring.any())
    fresh = ops.steplog_append(loss4, lr, grad[:n], theta[:n], ws, cursor, capacity=3)   # and the form that allocates the ring
    assert tuple(fresh.shape) == (3, 8) and fresh.dtype == torch.int32 and int(cursor.item()) == 1 and bool(fresh[0].any())
    memcheck.assert_guards()


# ------------------------------------------------------------------------------------------------ the learner
BATCHES = [[0, 1], [2, 3], [1, 2], [3, 0], [0, 2], [1, 3]]
RATES = [None, None, 2e-3, 2e-3, 5e-4, None]


@pytest.mark.parametrize("optimizer,precision", [("sgd", "fp32"), ("adam", "fp32"), ("sgd", "bf16")])
def test_learner_log_equals_what_a_synchronising_host_reads(optimizer, precision):
    from mliis_amd import metaseg
    from mliis_amd import steplog as S
    from mliis_amd._lib import MliisError, steplog_lib
    from mliis_amd.learner import Learner
    mk = lambda cap: Learner(image_size=H, rsd=[2, 4], drop_connect=False, optimizer=optimizer, matmul_precision=precision, seed=5,   # noqa: E731
                             use_graph=True, learning_rate=1e-3, step_log=cap)
    L8, L4, L0 = mk(8), mk(4), mk(0)
    assert L0.step_log == 0 and L0._log_ring is None and L0._log_cursor is None and L0._log_ws is None and tuple(L8._log_ring.shape) == (8, 8)
    x, y = metaseg.synthetic_task(4, H, seed=11)
    for L in (L8, L4, L0):
        L.load_task(x, y)
    seen = []
    for k, (b, lr) in enumerate(zip(BATCHES, RATES)):
        for L in (L8, L4, L0):
            steplog_lib.trace = []
            try:
                L.inner_step(b, lr=lr)
                calls = [name for name, _ in steplog_lib.trace]
            finally:
                steplog_lib.trace = None
            if k == 0:      # the eager step: one more launch with a log, none without
                assert calls == (["mliis_steplog_append"] if L.step_log else [])
        L8.synchronize()   # what a host without the log would have to do after every step
        g = L8.gradients_packed().cpu().numpy()
        seen.append((L8.last_loss.cpu().numpy().copy(), L8.lr_dev.cpu().numpy().copy(), np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2))),
                     np.abs(g).max()))
    assert L8.plans[2].graphs and L8.plans[2].steps_run == 6      # steps 3 to 6 were replays of one captured graph
    assert L8.step_log_pending() == 6
    r, dropped = L8.read_step_log()
    assert r.dtype == S.RECORD_DTYPE and len(r) == 6 and dropped == 0
    for k, (loss, lr, l2, amax) in enumerate(seen):
        print("step {} loss {!r} grad_l2: device {!r}, host float64 {!r}".format(k, r["loss"][k], r["grad_l2"][k], l2))
        assert r["loss"][k].tobytes() == loss[0].tobytes() and r["ce"][k].tobytes() == loss[1].tobytes() and r["iou"][k].tobytes() == loss[2].tobytes()
        assert r["lr"][k].tobytes() == lr[0].tobytes() == np.float32(1e-3 if RATES[k] is None else RATES[k]).tobytes()
        assert abs(float(r["grad_l2"][k]) - float(l2)) <= float(np.spacing(l2)) and l2 > 0
        assert r["grad_absmax"][k].tobytes() == np.float32(amax).tobytes()
        assert int(r["grad_nonfinite"][k]) == 0 and int(r["theta_nonfinite"][k]) == 0
    assert len(set(r["loss"].tolist())) == 6                      # six different steps, not one record six times
    again, dropped = L8.read_step_log()
    assert len(again) == 0 and dropped == 0 and L8.step_log_pending() == 0
    # a ring of four keeps the last four and says what it lost
    r4, dropped = L4.read_step_log()
    assert dropped == 2 and r4.tobytes() == r[2:].tobytes()
    # the twin without a log: the same parameters bit for bit, and nothing to read
    assert memcheck.bits_equal(L0.export_trainable(), L8.export_trainable()) and memcheck.bits_equal(L0.export_bn(), L8.export_bn())
    with pytest.raises(MliisError, match="step_log=0"):
        L0.read_step_log()
    # skip_step_log forgets without reading
    L8.inner_step(BATCHES[0])
    L8.skip_step_log()
    L8.inner_step(BATCHES[1])
    r1, dropped = L8.read_step_log()
    assert len(r1) == 1 and dropped == 0 and np.isfinite(r1["loss"][0])
    for L in (L8, L4, L0):
        L.close()


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
    with contextlib.redirect_stdout(io.StringIO()) as buf:
        out = fn(*a, **kw)
    return out, buf.getvalue()


def _learner(optimizer="sgd", seed=1):
    from mliis_amd.learner import Learner
    return Learner(image_size=H, rsd=[2, 4], drop_connect=False, optimizer=optimizer, seed=seed, use_graph=True, learning_rate=5e-3, step_log=64)


def test_summary_over_a_lane_equals_the_task_by_task_summary():
    from mliis_amd.reptile import Gecko
    tasks = _device_tasks()
    rows, thetas = [], []
    for n_lanes in (0, 1):
        L, lanes = _learner(), [_learner(seed=50) for _ in range(n_lanes)]
        meta, _ = _quiet(Gecko, L, rng_mode="per_task", seed=9, lanes=lanes, step_log=True)
        for _ in range(2):
            _quiet(meta.train_step, tasks, **STEP)
            rows.append(meta.inner_loop_summary)
        assert meta._lanes_in_use() == bool(n_lanes)
        thetas.append(L.export_trainable())
        for ln in [L] + lanes:
            ln.close()
    assert rows[0] == rows[2] and rows[1] == rows[3] and rows[0] != rows[1]       # bit for bit: the rows hold the floats themselves
    assert rows[0]["tasks"] == 2 and rows[0]["steps"] == 4 and rows[0]["nonfinite_steps"] == 0 and rows[1]["meta_iter"] == 1
    assert rows[0]["loss_first"] > 0 and rows[0]["grad_l2_first"] > 0 and rows[0]["lr"] == float(np.float32(5e-3))
    assert memcheck.bits_equal(thetas[0], thetas[1])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_guard_on_a_task_with_a_nan_pixel(optimizer):
    """One NaN pixel in the first image of a task: ordinary arithmetic carries it into the batch statistics, the loss and every gradient."""
    from mliis_amd import metaseg
    from mliis_amd import steplog as S
    from mliis_amd.reptile import Gecko, _task_rng
    good, tasks = _device_tasks(), _device_tasks(nan_in=(1,))
    # a seed under which task 0 of meta-iteration 0 draws the clean task and task 1 the damaged one (sample_task's first draw)
    seed = next(s for s in range(200) if [_task_rng(s, 0, t).sample(list(tasks), 1)[0].name for t in (0, 1)] == ["t0", "t1"])
    # the step of task 1 whose batch first holds shot 0: the draws of Gecko._sample and _batches, replayed
    rng = _task_rng(seed, 0, 1)
    metaseg.sample_task(tasks, 4, rng)
    first = next(j for j, b in enumerate(metaseg.mini_batch_indices(4, 2, 2, False, rng)) if 0 in b)
    L = _learner(optimizer)
    theta0, bn0 = L.export_trainable(), L.export_bn()
    meta, _ = _quiet(Gecko, L, rng_mode="per_task", seed=seed, on_divergence="skip")
    _, out = _quiet(meta.train_step, tasks, **STEP)
    row = meta.inner_loop_summary
    assert row["skipped"] is True and row["first_nonfinite"] == {"task": 1, "step": first} and row["nonfinite_steps"] == 2 - first
    assert "skipped" in out and meta.meta_iter == 1 and meta.skipped_meta_iters == 1
    assert memcheck.bits_equal(L.export_trainable(), theta0) and memcheck.bits_equal(L.export_bn(), bn0)
    assert len(L.read_step_log()[0]) == 0                                         # (the guard has read everything)
    # nothing of it is left in the learner (Adam: the second moments the NaN gradient went into were put back): a clean iteration follows
    meta, _ = _quiet(Gecko, L, rng_mode="per_task", seed=seed, on_divergence="skip")
    _quiet(meta.train_step, good, **STEP)
    row = meta.inner_loop_summary
    assert row["skipped"] is False and row["nonfinite_steps"] == 0 and np.isfinite(row["loss_last"]) and meta.skipped_meta_iters == 0
    theta1, bn1 = L.export_trainable(), L.export_bn()
    assert not memcheck.bits_equal(theta1, theta0) and bool(torch.isfinite(theta1).all()) and bool(torch.isfinite(bn1).all())
    # abort: raised before the update
    meta, _ = _quiet(Gecko, L, rng_mode="per_task", seed=seed, on_divergence="abort")
    with pytest.raises(S.DivergenceError, match="task 1 step {}".format(first)), contextlib.redirect_stdout(io.StringIO()):
        meta.train_step(tasks, **STEP)
    assert meta.meta_iter == 0
    assert memcheck.bits_equal(L.export_trainable(), theta1) and memcheck.bits_equal(L.export_bn(), bn1)
    # "off" logs the same steps and lets the update through, as a run without the option does
    L2 = _learner(optimizer)
    meta, _ = _quiet(Gecko, L2, rng_mode="per_task", seed=seed, step_log=True)
    _quiet(meta.train_step, tasks, **STEP)
    assert meta.inner_loop_summary["skipped"] is False and meta.inner_loop_summary["first_nonfinite"] == {"task": 1, "step": first}
    assert not bool(torch.isfinite(L2.export_trainable()).all())
    for ln in (L, L2):
        ln.close()
