"""What the inner loop's step log costs: inner-loop images/s at config 2 of BASELINE.json (EfficientLab-6-3, 224x224, meta-batch 1, 5 shots,
8 inner steps of batch 8, fp32, SGD, one MI355X) without and with step_log -- the extra launch at the tail of every step AND the one read of
the ring per meta-iteration, i.e. what `--inner-loop-log` adds to a run -- and, to tell the two apart, with the launch alone (a learner that
logs and a meta-learner that never reads: append_only).  One GPU process, three learners built once; every setting is timed
--repeats times, the settings alternating so that drift falls on both; host clock around --steps meta-steps that end in a device
synchronise, after --warmup untimed ones.  Every repeat runs under its own time limit (SIGALRM with the default action: a repeat that
exceeds --limit seconds ends the process instead of hanging it).

    python tools/bench_steplog.py [--steps 20] [--warmup 3] [--repeats 3] [--limit 120] [--tree DIR] [--json out.json]

--tree DIR imports mliis_amd from another checkout (the same tool on the parent commit: a Learner that does not know step_log is timed
without it only).  There is no CPU path: without a GPU this fails."""
import argparse
import contextlib
import io
import json
import os
import signal
import statistics
import sys
import time

import torch


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds one repeat (and each learner's build + warm-up) may take")
    p.add_argument("--tree", default=None, help="checkout to import mliis_amd from (default: the one this file is in)")
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_steplog needs an MI355X: there is no CPU path and no number without one")
    import mliis_amd
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import DeviceTask, synthetic_task
    from mliis_amd.reptile import Gecko
    assert os.path.dirname(os.path.abspath(mliis_amd.__file__)) == os.path.join(root, "mliis_amd"), mliis_amd.__file__
    dev = torch.device("cuda", 0)
    shots, inner_iters, inner_batch, size = 5, 8, 8, 224
    tasks = []
    for i in range(8):
        x, y = synthetic_task(shots, size, seed=i)
        tasks.append(DeviceTask("synthetic_%d" % i, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)))

    def limited(fn):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(a.limit)
        try:
            return fn()
        finally:
            signal.alarm(0)

    def build(step_log, read=True):
        kw = dict(step_log=64) if step_log else {}
        L = Learner(image_size=size, rsd=(2, 4), learning_rate=1e-3, optimizer="sgd", seed=0, device=dev, max_shots=16, **kw)
        with contextlib.redirect_stdout(io.StringIO()):
            meta = Gecko(L, rng_mode="per_task", seed=0, **(dict(step_log=True) if (step_log and read) else {}))
        return L, meta

    def meta_steps(meta, n):
        for _ in range(n):
            meta.train_step(tasks, num_shots=shots, inner_batch_size=inner_batch, inner_iters=inner_iters, replacement=False, meta_step_size=0.1,
                            meta_batch_size=1)

    settings = {"without_step_log": limited(lambda: build(False))}
    try:
        settings["append_only"] = limited(lambda: build(True, read=False))   # the launch in every step, the ring never read
        settings["with_step_log"] = limited(lambda: build(True))
    except TypeError as e:       # a checkout from before the option
        print("this checkout's Learner has no step_log ({}): timed without it only".format(e), file=sys.stderr)
    for L, meta in settings.values():
        limited(lambda: (meta_steps(meta, a.warmup), L.synchronize()))
    values = {k: [] for k in settings}
    for _ in range(a.repeats):
        for name, (L, meta) in settings.items():
            def timed():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                meta_steps(meta, a.steps)
                torch.cuda.synchronize()
                return time.perf_counter() - t0
            dt = limited(timed)
            values[name].append(inner_iters * inner_batch * a.steps / dt)
    out = dict(config="BASELINE.json configs[1]: 224x224, meta-batch 1, 5-shot x 8 inner steps of batch 8, fp32, SGD, 1 GPU", unit="images/s",
               steps=a.steps, warmup=a.warmup, repeats=a.repeats, tree=root, device=torch.cuda.get_device_name(0),
               images_per_s={k: dict(median=statistics.median(v), min=min(v), max=max(v), repeats=v) for k, v in values.items()})
    if "with_step_log" in settings:
        meta = settings["with_step_log"][1]
        out["last_summary"] = meta.inner_loop_summary
    for L, _ in settings.values():
        L.close()
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
