"""Concurrent lanes with on-device augmentation, host logic only: Gecko / FOMLIS on the CPU oracle learner with a stand-in for the
device augmenter that records what it is asked to make.  With lanes the draws (task sample, split / shuffles, per-sample recipes) must be
the ones of the task-by-task loop, every task's batches must reach the learner that steps on them, and the meta-update must not move."""
import random

import numpy as np
import pytest
import torch

from mliis_amd import augment, metaseg
from mliis_amd.reptile import FOMLIS, Gecko
from oracle import efficientlab_ref as R

H = 32


class _Log:
    """Per-task records in the order the tasks were made resident (= task order, with lanes or without)."""

    def __init__(self):
        self.tasks = []


class _AugOracle(R.OracleLearner):
    """OracleLearner + the augmentation surface of mliis_amd.learner.Learner.  augment_batch makes no pixels: it records
    (src_idx, recipes) under the resident task and hands the shots back, so the steps run on the raw examples."""

    def __init__(self, log, augment_batch_capacity=0, extendable=True, **kw):
        super().__init__(image_size=H, dtype=torch.float64, lr=1e-2, drop_connect=False, **kw)
        self.aug_capacity = augment_batch_capacity
        self.extendable = extendable
        self.log, self.cur, self.n_aug, self.n_steps = log, None, 0, 0

    def reserve_augment_capacity(self, n):
        if not self.extendable:
            raise ValueError("this learner has already stepped")
        self.aug_capacity = max(self.aug_capacity, int(n))

    def load_task(self, images, labels):
        super().load_task(images, labels)
        self.cur = []
        self.log.tasks.append(self.cur)

    def augment_batch(self, src_idx, recipes):
        assert len(src_idx) <= self.aug_capacity
        self.cur.append(("augment", [int(i) for i in src_idx], recipes))
        self.n_aug += 1
        return [int(i) for i in src_idx]

    def inner_step(self, x, *a, **kw):
        self.cur.append(("step", [int(i) for i in x]))
        self.n_steps += 1
        return super().inner_step(x, *a, **kw)


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def _tasks(n, shots):
    out = []
    for i in range(n):
        x, y = metaseg.synthetic_task(shots, H, seed=70 + i, block=4)
        out.append(metaseg.DeviceTask("t%d" % i, torch.tensor(x), torch.tensor(y)))
    return out


def _reset_host_generators(seed):
    random.seed(seed)
    np.random.seed(seed)
    augment._SHARED_ORDER[:] = list(augment.PRISTINE_ORDER)   # process-wide and persistent in "reference" mode


def _run(tasks, fomaml, rng_mode, lanes_kw, evaluate=True, meta_steps=2):
    """Meta-steps over 4 tasks (with 2 lanes: a full group and a ragged one) and one evaluation over 2.  lanes_kw: constructor keywords
    of every lane."""
    _reset_host_generators(21)
    log = _Log()
    A = _AugOracle(log, augment_batch_capacity=8, seed=3)
    lanes = [_AugOracle(log, seed=90 + k, **kw) for k, kw in enumerate(lanes_kw)]
    kw = dict(rng_mode=rng_mode, seed=4, lanes=lanes, augment="device", aug_rate=0.7)
    meta = FOMLIS(A, train_shots=6, tail_shots=2, **kw) if fomaml else Gecko(A, **kw)
    for _ in range(meta_steps):
        meta.train_step(tasks, num_shots=6, inner_batch_size=4, inner_iters=3, meta_step_size=0.5, meta_batch_size=4)
    n_train = len(log.tasks)
    ev = meta.evaluate(list(tasks[:2]), num_shots=3, test_shots=2, inner_batch_size=2, inner_iters=2, eval_all_tasks=True) if evaluate else None
    return dict(theta=A.export_trainable().clone(), bn=A.export_bn().clone(), ev=ev, tasks=log.tasks, n_train=n_train, main=A, lanes=lanes,
                meta=meta, draws=(random.random(), float(np.random.rand())))


@pytest.mark.parametrize("rng_mode", ["per_task", "reference"])
@pytest.mark.parametrize("fomaml", [False, True])
def test_lanes_with_device_augmentation_equal_task_by_task(fomaml, rng_mode):
    tasks = _tasks(4, 6)
    a = _run(tasks, fomaml, rng_mode, [])
    b = _run(tasks, fomaml, rng_mode, [dict(augment_batch_capacity=8), dict()])   # (the second lane is extended by Gecko)
    assert b["meta"]._lanes_in_use() and all(ln.aug_capacity >= 8 for ln in b["lanes"])
    # the lanes adapted tasks and made augmented batches (on the code before this feature they sit idle)
    assert all(ln.n_steps > 0 and ln.n_aug > 0 for ln in b["lanes"]), [(ln.n_steps, ln.n_aug) for ln in b["lanes"]]
    # per task, the same sequence of (src_idx, recipes) and of stepped indices
    assert len(a["tasks"]) == len(b["tasks"]) == 2 * 4 + 2
    for t, (ta, tb) in enumerate(zip(a["tasks"], b["tasks"])):
        assert _same(ta, tb), t
    assert any(len(r) >= 2 for task in a["tasks"] for rec in task if rec[0] == "augment" for r in rec[2] if r is not None)
    if fomaml:   # the raw tail comes last: plain shot indices, never through augment_batch
        for task in a["tasks"][:a["n_train"]]:
            assert task[-1][0] == "step" and len(task[-1][1]) == 2 and task[-2][0] == "step"
    assert torch.equal(a["theta"], b["theta"]) and torch.equal(a["bn"], b["bn"])
    assert a["ev"] == b["ev"]
    assert a["draws"] == b["draws"]   # the global generators were left at the same position (consumed only in "reference" mode)


def test_a_lane_that_cannot_be_extended_falls_back_to_task_by_task(capsys):
    tasks = _tasks(4, 6)
    a = _run(tasks, False, "per_task", [], evaluate=False, meta_steps=1)
    b = _run(tasks, False, "per_task", [dict(extendable=False)], evaluate=False, meta_steps=1)
    assert "one at a time" in capsys.readouterr().out
    assert not b["meta"]._lanes_in_use()
    assert b["lanes"][0].n_steps == 0 and b["lanes"][0].aug_capacity == 0
    assert torch.equal(a["theta"], b["theta"]) and torch.equal(a["bn"], b["bn"])
    # a lane without the method at all: the same
    log = _Log()
    plain = R.OracleLearner(image_size=H, seed=5, dtype=torch.float64, lr=1e-2, drop_connect=False)
    g = Gecko(_AugOracle(log, augment_batch_capacity=8, seed=3), rng_mode="per_task", lanes=[plain], augment="device")
    assert not g._lanes_in_use()
    # the main learner still needs the capacity
    with pytest.raises(ValueError):
        Gecko(_AugOracle(log, seed=3), rng_mode="per_task", lanes=[_AugOracle(log, augment_batch_capacity=8, seed=4)], augment="device")
