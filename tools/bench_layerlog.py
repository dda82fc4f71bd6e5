"""What the inner loop's per-tensor log costs: inner-loop images/s at config 2 of BASELINE.json (EfficientLab-6-3, 224x224, meta-batch 1,
5 shots, 8 inner steps of batch 8, fp32, SGD, one MI355X)
  without_step_log   Learner() and Gecko() as always;
  with_step_log      --inner-loop-log alone: Learner(step_log=64), Gecko(step_log=True);
  layer_launches     the per-tensor log's launches and no ring read: Learner(step_log=64, layer_log=True) and a Gecko whose interval never
                     comes round after the warm-up -- two more launches in every step's graph, one delta per task, the step log read as above;
  with_layer_log     --inner-loop-layer-log at its default interval of 100 meta-iterations.
One GPU process, the learners built once; every setting is timed --repeats times, the settings alternating so that drift falls on all;
host clock around --steps meta-steps that end in a device synchronise, after --warmup untimed ones.  Every repeat runs under its own time
limit (SIGALRM with the default action: a repeat that exceeds --limit seconds ends the process instead of hanging it).

    python tools/bench_layerlog.py [--steps 100] [--warmup 5] [--repeats 3] [--limit 120] [--tree DIR] [--json out.json]

--tree DIR imports mliis_amd from another checkout (the same tool on the parent commit: a Learner that does not know layer_log is timed in
the settings it has).  There is no CPU path: without a GPU this fails."""
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
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds one repeat (and each learner's build + warm-up) may take")
    p.add_argument("--tree", default=None, help="checkout to import mliis_amd from (default: the one this file is in)")
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_layerlog needs an MI355X: there is no CPU path and no number without one")
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

    def build(learner_kw, meta_kw):
        L = Learner(image_size=size, rsd=(2, 4), learning_rate=1e-3, optimizer="sgd", seed=0, device=dev, max_shots=16, **learner_kw)
        with contextlib.redirect_stdout(io.StringIO()):
            meta = Gecko(L, rng_mode="per_task", seed=0, **meta_kw)
        return L, meta

    def meta_steps(meta, n):
        for _ in range(n):
            meta.train_step(tasks, num_shots=shots, inner_batch_size=inner_batch, inner_iters=inner_iters, replacement=False, meta_step_size=0.1,
                            meta_batch_size=1)

    never = a.warmup + a.steps * a.repeats + 1   # an interval that comes round at meta-iteration 0 (inside the warm-up) and never again
    settings = {"without_step_log": limited(lambda: build({}, {}))}
    for name, lkw, mkw in (("with_step_log", dict(step_log=64), dict(step_log=True)),
                           ("layer_launches", dict(step_log=64, layer_log=True), dict(step_log=True, layer_log=True, layer_log_interval=never)),
                           ("with_layer_log", dict(step_log=64, layer_log=True), dict(step_log=True, layer_log=True, layer_log_interval=100))):
        try:
            settings[name] = limited(lambda: build(lkw, mkw))
        except TypeError as e:       # a checkout from before the option
            print("this checkout has no {} ({}): not timed".format(name, e), file=sys.stderr)
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
    if "with_layer_log" in settings:
        L, meta = settings["with_layer_log"]
        out["tensors"] = len(L.layer_log_names)
        out["layer_rows_built"] = [name for name in ("layer_launches", "with_layer_log")
                                   if settings[name][1].inner_loop_layers_summary is not None]
    for L, _ in settings.values():
        L.close()
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
