"""Concurrent lanes with on-device augmentation (Gecko / FOMLIS(lanes=..., augment="device")): the tasks of a meta-batch adapted
several at a time on learners of their own, every learner augmenting its own batches on its own stream, give the meta-update and the
evaluation of the task-by-task loop bit for bit -- and the lanes really do the work (without that the equalities would hold trivially,
the fallback being the task-by-task loop).  64x64 images, 10 shots per task, no drop-connect / dropout, captured graphs, fp32."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _tasks(n, seed0):
    from mliis_amd.metaseg import DeviceTask, synthetic_task
    dev = torch.device("cuda", 0)
    out = []
    for i in range(n):
        x, y = synthetic_task(10, H, seed=seed0 + i)
        out.append(DeviceTask("t%d" % i, torch.tensor(x).to(dev), torch.tensor(y).to(dev)))
    return out


def _learner(seed, slots=16, **kw):
    from mliis_amd.learner import Learner
    return Learner(image_size=H, seed=seed, use_graph=True, drop_connect=False, augment_batch_capacity=slots, **kw)


def _spy(ln):
    """Record, per resident task, the indices of every inner step and the recipes of every augmented batch of this learner."""
    rec = {"tasks": [], "recipes": []}
    load, step, aug = ln.load_task, ln.inner_step, ln.augment_batch

    def load_task(images, labels):
        rec["tasks"].append([])
        return load(images, labels)

    def inner_step(idx, *a, **kw):
        rec["tasks"][-1].append([int(i) for i in idx])
        return step(idx, *a, **kw)

    def augment_batch(src_idx, recipes):
        rec["recipes"].extend(recipes)
        return aug(src_idx, recipes)

    ln.load_task, ln.inner_step, ln.augment_batch = load_task, inner_step, augment_batch
    return rec


def _reset_host_generators(seed):
    from mliis_amd import augment
    random.seed(seed)
    np.random.seed(seed)
    augment._SHARED_ORDER[:] = list(augment.PRISTINE_ORDER)   # "reference" mode: process-wide, persistent across meta-learners


def _meta_run(tasks, fomaml, rng_mode, lanes, main=None, meta_steps=2):
    """Two meta-steps of 3 tasks; returns (theta, bn, position of the global generators, per-learner records, the meta-learner)."""
    from mliis_amd.reptile import FOMLIS, Gecko
    _reset_host_generators(13)
    L = main or _learner(1)
    recs = [_spy(ln) for ln in [L] + list(lanes)]
    kw = dict(rng_mode=rng_mode, seed=9, lanes=list(lanes), augment="device", aug_rate=0.7)
    meta = FOMLIS(L, train_shots=10, tail_shots=5, **kw) if fomaml else Gecko(L, **kw)
    for _ in range(meta_steps):
        meta.train_step(tasks, num_shots=10, inner_batch_size=4, inner_iters=3, meta_step_size=0.5, meta_batch_size=3)
    st = L.export_all()
    out = (st["theta"].cpu().clone(), st["bn"].cpu().clone(), (random.random(), float(np.random.rand())), recs, meta)
    for ln in [L] + list(lanes):
        ln.close()
    return out


def _check_lane_use(recs, max_shots, fomaml):
    lane_recs = recs[1:]
    # task t of a meta-batch of 3 goes to learner t mod (number of learners): every lane that has a task to take took it in both
    # meta-steps and stepped on it (3 tasks on 4 learners leave the last lane without one)
    for k, r in enumerate(recs):
        assert len(r["tasks"]) == 2 * len(range(k, 3, len(recs))), (k, len(r["tasks"]))
        assert all(len(t) == 3 for t in r["tasks"]), "learner %d was given a task and did not run its inner steps" % k
    assert sum(len(r["tasks"]) for r in lane_recs) > 0, "no lane executed an inner step"
    assert any(i >= max_shots for r in lane_recs for t in r["tasks"] for idx in t for i in idx), "no lane stepped on augmented slots"
    assert any(rc is not None and len(rc) >= 2 for r in recs for rc in r["recipes"]), "no recipe with two or more stages"
    if fomaml:   # the raw tail: plain shot indices, five of them, last
        for r in recs:
            for t in r["tasks"]:
                assert len(t) == 3 and len(t[-1]) == 5 and all(i < max_shots for i in t[-1]), t


@pytest.mark.parametrize("fomaml", [False, True])
def test_meta_step_with_lanes_and_device_augmentation_equals_task_by_task(fomaml):
    """rng_mode="per_task": 3 tasks on 1, 2 (ragged last group) and 4 (all at once) learners."""
    _need_gpu()
    tasks = _tasks(4, 20)
    a = _meta_run(tasks, fomaml, "per_task", [])
    assert any(i >= 16 for t in a[3][0]["tasks"] for idx in t for i in idx)
    for n_lanes in (1, 3):
        b = _meta_run(tasks, fomaml, "per_task", [_learner(50 + k) for k in range(n_lanes)])
        assert b[4]._lanes_in_use()
        _check_lane_use(b[3], 16, fomaml)
        assert torch.equal(a[0], b[0]), (n_lanes, float((a[0] - b[0]).abs().max()))
        assert torch.equal(a[1], b[1]), (n_lanes, float((a[1] - b[1]).abs().max()))


@pytest.mark.parametrize("fomaml", [False, True])
def test_meta_step_with_a_lane_in_reference_rng_mode(fomaml):
    """One rank, the global generators: the same update and the same number of draws taken from `random` and `numpy.random`."""
    _need_gpu()
    tasks = _tasks(4, 20)
    a = _meta_run(tasks, fomaml, "reference", [])
    b = _meta_run(tasks, fomaml, "reference", [_learner(50)])
    _check_lane_use(b[3], 16, fomaml)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), float((a[0] - b[0]).abs().max())
    assert a[2] == b[2]


@pytest.mark.parametrize("device_metrics", [False, True])
@pytest.mark.parametrize("transductive", [False, True])
def test_evaluation_with_a_lane_and_device_augmentation_equals_task_by_task(transductive, device_metrics):
    _need_gpu()
    from mliis_amd.reptile import Gecko
    tasks = _tasks(3, 40)
    L, lane = _learner(2, learning_rate=5e-3), _learner(77, learning_rate=5e-3)
    rec = _spy(lane)
    before = L.export_all()
    res = []
    for lanes in ((), (lane,)):
        _reset_host_generators(11)
        g = Gecko(L, rng_mode="reference", transductive=transductive, lanes=lanes, augment="device", aug_rate=0.7,
                  device_metrics=device_metrics)
        res.append((g.evaluate(list(tasks), num_shots=5, inner_batch_size=4, inner_iters=3, eval_all_tasks=True),
                    random.random(), float(np.random.rand())))
    after = L.export_all()
    print("evaluate", transductive, device_metrics, res)
    assert res[0][0][1] == res[1][0][1] and res[0][0][0] == res[1][0][0], (res[0], res[1])
    assert len(res[0][0][1]) == 3
    assert res[0][1:] == res[1][1:]              # the same draws were taken from both global generators
    assert torch.equal(before["theta"], after["theta"]) and torch.equal(before["bn"], after["bn"])
    assert sum(len(t) for t in rec["tasks"]) == 3 and len(rec["tasks"]) == 1     # the lane fine-tuned the second task
    assert any(i >= 16 for t in rec["tasks"] for idx in t for i in idx)
    L.close()
    lane.close()


def test_lanes_built_without_augmentation_slots_are_extended():
    """What a caller builds that knows nothing of the augmenter: lanes with no batch slots.  Gecko gives them the main learner's
    (Learner.reserve_augment_capacity); a lane that cannot be extended any more -- it has stepped -- makes Gecko adapt task by task."""
    _need_gpu()
    tasks = _tasks(4, 20)
    a = _meta_run(tasks, False, "per_task", [])
    lane = _learner(50, slots=0)
    assert lane.aug_capacity == 0 and lane.shots_x.shape[0] == lane.max_shots
    x, y = tasks[0].sample(10)
    lane.load_task(x, y)     # resident shots survive the re-allocation
    b = _meta_run(tasks, False, "per_task", [lane])
    assert lane.aug_capacity == 16 and lane.shots_x.shape[0] == lane.max_shots + 16 and lane.shots_y.shape[0] == lane.max_shots + 16
    assert b[4]._lanes_in_use()
    _check_lane_use(b[3], 16, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), float((a[0] - b[0]).abs().max())

    stepped = _learner(51, slots=0)
    stepped.load_task(x, y)
    stepped.synchronize()
    kept = stepped.shots_x[:10].clone()
    stepped.inner_step([0, 1, 2, 3])
    with pytest.raises(ValueError):
        stepped.reserve_augment_capacity(16)
    assert stepped.aug_capacity == 0
    c = _meta_run(tasks, False, "per_task", [stepped])
    assert not c[4]._lanes_in_use()
    assert len(c[3][1]["tasks"]) == 0       # the lane was given no task
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])

    fresh = _learner(52, slots=0)           # contents kept: the shots read back from the larger allocation
    fresh.load_task(x, y)
    fresh.reserve_augment_capacity(8)
    assert fresh.aug_capacity == 8 and torch.equal(fresh.shots_x[:10], kept) and not bool(fresh.shots_x[10:].any())
    fresh.close()


@pytest.mark.parametrize("on_host,learners", [(False, 2), (True, 1)])
def test_command_line_builds_lanes_for_device_augmentation(tmp_path, on_host, learners):
    """`run_metasegnet.py --augment --concurrent-tasks 2`: two learners adapt the tasks; with --augment-on-host one, and it says why."""
    _need_gpu()
    argv = ["--synthetic-tasks", "6", "--image_size", "64", "--rsd", "2", "4", "--sgd", "--augment", "--aug_rate", "0.7", "--concurrent-tasks", "2",
            "--shots", "3", "--inner-batch", "4", "--inner-iters", "3", "--meta-batch", "2", "--meta-iters", "2", "--eval-interval", "0",
            "--eval-samples", "2", "--eval-iters", "2", "--eval-batch", "3", "--learning-rate", "0.005", "--skip-train-task-eval",
            "--checkpoint", str(tmp_path / "ck")] + (["--augment-on-host", "--augment-workers", "0"] if on_host else [])
    p = subprocess.run([sys.executable, os.path.join(ROOT, "run_metasegnet.py")] + argv, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0
    assert "Mean IoU over all meta-test tasks:" in p.stdout
    assert "Adapting tasks on {} learner(s).".format(learners) in p.stdout
    assert ("--augment-on-host adapts one task at a time" in p.stdout) == on_host
