"""Times making a task resident -- Learner.load_task for 10 shots -- from the four forms a task can have, and one meta-iteration over
lanes fed by two of them.  One GPU process; host clock around work that ends in a synchronise of the learner's stream; every shape warmed
up before its timed window; the cases alternate inside every round so that drift falls on all of them.

    python tools/bench_taskload.py [--shots 10] [--size 224] [--big 384] [--rounds 30] [--meta-rounds 5] [--json out.json]

  (a) host numpy float32 arrays       what --data-dir hands to load_task by default (tfrecord.ShardTask): a pageable upload
  (b) device float32 tensors          metaseg.DeviceTask (--synthetic-tasks, bench.py): a device-to-device copy
  (c) ByteTask at the stored size     --resident-dataset: one expansion launch from the resident bytes
  (d) ByteTask --size -> --big        the same launch resampling, on a learner built at --big
and one meta-iteration (Reptile, SGD, 8 inner steps of batch 8) of --meta-batch 8 over 4 concurrent learners on tasks of form (a) and (c).
There is no CPU path: without a GPU this fails."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class HostTask:
    """A task as tfrecord.ShardTask holds it after decoding: host float32 arrays, sample() = the first examples."""

    def __init__(self, name, images, labels):
        self.name, self.images, self.labels, self.batch_size = name, images, labels, int(images.shape[0])

    def sample(self, num_images):
        return self.images[:num_images], self.labels[:num_images]


def _stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--shots", type=int, default=10)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--big", type=int, default=384)
    p.add_argument("--rounds", type=int, default=30)
    p.add_argument("--meta-rounds", type=int, default=5)
    p.add_argument("--meta-batch", type=int, default=8)
    p.add_argument("--concurrent-tasks", type=int, default=4)
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_taskload needs an MI355X: there is no CPU path and no number without one")
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import ByteTask, DeviceTask, expand_bytes_host, synthetic_task_bytes
    from mliis_amd.reptile import Gecko
    dev = torch.device("cuda", 0)
    S, H = a.shots, a.size

    def forms(seed):
        xb, mb = synthetic_task_bytes(S, H, seed=seed)
        x, y = expand_bytes_host(xb, mb, H, H)
        name = "t%d" % seed
        bt = ByteTask(name, torch.from_numpy(xb).to(dev), torch.from_numpy(mb).to(dev), H)
        big = ByteTask(name, bt.images_u8, bt.masks_u8, a.big)
        return HostTask(name, x, y), DeviceTask(name, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)), bt, big

    mk = lambda size, seed: Learner(image_size=size, seed=seed, optimizer="sgd", drop_connect=False, max_shots=max(16, S))   # noqa: E731
    # (drop-connect off: every lane draws its masks from its own generator, and the two forms are also compared bit for bit below)
    L, Lbig = mk(H, 0), mk(a.big, 0)
    host, devf, bt, big = forms(0)
    cases = [("a_host_float_arrays", L, host), ("b_device_float_tensors", L, devf), ("c_byte_task_same_size", L, bt),
             ("d_byte_task_%d_to_%d" % (H, a.big), Lbig, big)]
    times = {name: [] for name, _, _ in cases}
    for r in range(3 + a.rounds):                      # three warm-up rounds, then the timed ones; the cases alternate
        for name, ln, task in cases:
            images, labels = task.sample(S)
            ln.synchronize()
            t0 = time.perf_counter()
            ln.load_task(images, labels)
            ln.synchronize()
            if r >= 3:
                times[name].append((time.perf_counter() - t0) * 1e3)
    # the forms agree: (c) leaves the floats (a) leaves
    L.load_task(*host.sample(S))
    L.synchronize()
    ref = (L.shots_x[:S].clone(), L.shots_y[:S].clone())
    L.load_task(*bt.sample(S))
    L.synchronize()
    same = bool(torch.equal(ref[0], L.shots_x[:S]) and torch.equal(ref[1], L.shots_y[:S]))
    out = dict(shots=S, size=H, big=a.big, rounds=a.rounds, load_task_ms={k: _stats(v) for k, v in times.items()}, c_equals_a_bitwise=same,
               float_bytes_per_task=S * H * H * 20, stored_bytes_per_task=S * H * H * 4)
    Lbig.close()
    del Lbig
    # one meta-iteration over the lanes, tasks of form (a) against tasks of form (c)
    lanes = [mk(H, 1000 * k) for k in range(1, a.concurrent_tasks)]
    sets = {"a_host_float_arrays": [], "c_byte_task_same_size": []}
    for i in range(a.meta_batch):
        h_, _, b_, _ = forms(100 + i)
        sets["a_host_float_arrays"].append(h_)
        sets["c_byte_task_same_size"].append(b_)
    with contextlib.redirect_stdout(io.StringIO()):
        meta = Gecko(L, rng_mode="per_task", seed=1, lanes=lanes)
    mtimes = {k: [] for k in sets}
    thetas = {}
    for r in range(2 + a.meta_rounds):                 # the first two iterations size the plans and capture the graphs
        for name, tasks in sets.items():
            meta.meta_iter = r                           # the same draws for both forms
            before = L.export_all()
            L.synchronize()
            t0 = time.perf_counter()
            meta.train_step(list(tasks), num_shots=S, inner_batch_size=8, inner_iters=8, meta_step_size=0.1, meta_batch_size=a.meta_batch)
            L.synchronize()
            if r >= 2:
                mtimes[name].append((time.perf_counter() - t0) * 1e3)
            thetas[name] = L.export_all()["theta"].clone()
            L.import_all(before)                       # both forms start every round from the same state
    out["meta_iteration_ms"] = {k: _stats(v) for k, v in mtimes.items()}
    out["meta_iteration"] = dict(meta_batch=a.meta_batch, concurrent_tasks=a.concurrent_tasks, inner_iters=8, inner_batch=8, rounds=a.meta_rounds,
                                 lanes_in_use=bool(meta._lanes_in_use()))
    out["meta_update_c_equals_a_bitwise"] = bool(torch.equal(thetas["a_host_float_arrays"], thetas["c_byte_task_same_size"]))
    for ln in [L] + lanes:
        ln.close()
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
