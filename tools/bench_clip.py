"""What the inner loop's gradient clipping costs: inner-loop images/s at config 2 of BASELINE.json (EfficientLab-6-3, 224x224, meta-batch 1,
5 shots, 8 inner steps of batch 8, fp32, SGD, one MI355X)
  without_flags      Learner() and Gecko() as always;
  clip_norm          --inner-clip-norm C: Learner(grad_clip=("norm", C)) -- two more launches in every step's graph, the ring never read;
  clip_ratio         --inner-clip-ratio LAMBDA: Learner(grad_clip=("ratio", LAMBDA, EPS)), likewise;
  with_step_log      --inner-loop-log alone: Learner(step_log=64), Gecko(step_log=True);
  clip_norm_log      --inner-clip-norm with --inner-loop-log: the clip's ring is read where the step ring is, once per meta-iteration;
  clip_ratio_log     --inner-clip-ratio with --inner-loop-log.
One GPU process per tree, the learners built once; every setting is timed --repeats times, the settings alternating so that drift falls on
all; host clock around --steps meta-steps that end in a device synchronise, after --warmup untimed ones.  Every repeat runs under its own
time limit (SIGALRM with the default action: a repeat that exceeds --limit seconds ends the process instead of hanging it).

    python tools/bench_clip.py [--steps 100] [--warmup 5] [--repeats 3] [--limit 120] [--tree DIR] [--json out.json]
    python tools/bench_clip.py --parent DIR --md profiles/clip.md [...]

--tree DIR imports mliis_amd from another checkout (the same tool on the parent commit: a Learner that does not know grad_clip is timed in
the settings it has).  --parent DIR (a built checkout of the parent commit) makes this process an orchestrator that never touches the GPU
itself: it starts one fresh child process after the other -- the parent commit, this tree, the parent commit again -- stops at the first
that fails, and writes the table of --md from their results.  There is no CPU path: without a GPU this fails."""
import argparse
import contextlib
import io
import json
import os
import signal
import statistics
import subprocess
import sys
import time

SETTINGS = ("without_flags", "clip_norm", "clip_ratio", "with_step_log", "clip_norm_log", "clip_ratio_log")


def measure(a):
    import torch
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip needs an MI355X: there is no CPU path and no number without one")
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

    norm, ratio = ("norm", a.clip_norm), ("ratio", a.clip_ratio, a.clip_ratio_eps)
    settings = {"without_flags": limited(lambda: build({}, {}))}
    for name, lkw, mkw in (("clip_norm", dict(grad_clip=norm), {}), ("clip_ratio", dict(grad_clip=ratio), {}),
                           ("with_step_log", dict(step_log=64), dict(step_log=True)),
                           ("clip_norm_log", dict(step_log=64, grad_clip=norm, clip_log=64), dict(step_log=True)),
                           ("clip_ratio_log", dict(step_log=64, grad_clip=ratio, clip_log=64), dict(step_log=True))):
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
               clip_norm=a.clip_norm, clip_ratio=a.clip_ratio, clip_ratio_eps=a.clip_ratio_eps, images_per_step=inner_batch,
               images_per_s={k: dict(median=statistics.median(v), min=min(v), max=max(v), repeats=v) for k, v in values.items()})
    # what the bounds did, from the rings (after the timing): share of the last rows that clipped, their smallest scale
    from_rings = {}
    for name, (L, _) in settings.items():
        if getattr(L, "grad_clip", None) is not None:
            rows, _ = L.read_clip_log()
            from_rings[name] = dict(rows=int(rows.shape[0]), records_per_row=int(rows.shape[1]), chunks=int(L._clip_table.nchunks),
                                    clip_frac=float(((rows["flags"] & 1) != 0).any(axis=1).mean()), scale_min=float(rows["scale"].min()),
                                    bypassed=int(((rows["flags"] & 2) != 0).any(axis=1).sum()))
    out["rings"] = from_rings
    for L, _ in settings.values():
        L.close()
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


def _cell(r, name):
    v = r["images_per_s"].get(name)
    return "-" if v is None else "{:.1f} ({:.1f}-{:.1f})".format(v["median"], v["min"], v["max"])


def orchestrate(a):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parent = os.path.abspath(a.parent)
    out_dir = os.path.dirname(os.path.abspath(a.md))
    os.makedirs(out_dir, exist_ok=True)
    runs = []
    for label, tree in (("parent commit, process 1", parent), ("this tree", here), ("parent commit, process 2", parent)):
        path = os.path.join(out_dir, ".bench_clip_{}.json".format(len(runs)))
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats),
               "--limit", str(a.limit), "--clip-norm", str(a.clip_norm), "--clip-ratio", str(a.clip_ratio), "--clip-ratio-eps",
               str(a.clip_ratio_eps), "--tree", tree, "--json", path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit * (2 + a.repeats) * len(SETTINGS))
        if r.returncode != 0:      # nothing more is started on the device after a process that failed
            raise SystemExit("{} failed ({}):\n{}".format(label, r.returncode, r.stderr[-3000:]))
        with open(path) as f:
            runs.append((label, json.loads(f.read())))
        os.remove(path)
        print("{}: {}".format(label, {k: round(v["median"], 1) for k, v in runs[-1][1]["images_per_s"].items()}), flush=True)
    (_, p1), (_, t), (_, p2) = runs
    per_step = t["images_per_step"]
    ms = lambda r, k: 1e3 * per_step / r["images_per_s"][k]["median"]   # noqa: E731  (ms per inner step)
    lines = ["# What inner-loop gradient clipping costs", "",
             "One MI355X, `tools/bench_clip.py`: config 2 of `BASELINE.json` (EfficientLab-6-3, 224², meta-batch 1, 5 shots, 8 inner SGD steps of",
             "batch 8, fp32, captured graphs), inner-loop images/s of `Gecko.train_step`. Host clock around {} meta-steps that end in a device".format(t["steps"]),
             "synchronise, after {} untimed ones; every setting {} times, the settings alternating. Three processes, one after the other: the".format(t["warmup"], t["repeats"]),
             "parent commit, this tree, the parent commit again (a parent from before `grad_clip` runs the two settings it has).", "",
             "    python tools/bench_clip.py --parent <built checkout of the parent commit> --md profiles/clip.md --steps {} --warmup {} --repeats {}".format(
                 t["steps"], t["warmup"], t["repeats"]), "",
             "`--inner-clip-norm {}`, `--inner-clip-ratio {}` with eps {}.".format(t["clip_norm"], t["clip_ratio"], t["clip_ratio_eps"]), "",
             "| setting | this tree: median (min-max) images/s | parent, process 1 | parent, process 2 |", "|---|---|---|---|"]
    for name in SETTINGS:
        lines.append("| `{}` | {} | {} | {} |".format(name, _cell(t, name), _cell(p1, name), _cell(p2, name)))
    off, a1, a2 = t["images_per_s"]["without_flags"], p1["images_per_s"]["without_flags"], p2["images_per_s"]["without_flags"]
    lo, hi = min(a1["min"], a2["min"]), max(a1["max"], a2["max"])
    inside = lo <= off["median"] <= hi
    lines += ["", "* **Flags off**: {:.1f} images/s (median) against {:.1f}-{:.1f} over the two processes of the parent commit (medians {:.1f} and {:.1f}): {}.".format(
        off["median"], lo, hi, a1["median"], a2["median"],
        "inside the spread between the two" if inside else "OUTSIDE the spread between the two ({:+.2f} % against their mean)".format(
            100 * (off["median"] / ((a1["median"] + a2["median"]) / 2) - 1)))]
    lines.append("* **The launches** (two per step in both modes, ring never read), per 8-image inner step against `without_flags` of the same process:")
    for name in ("clip_norm", "clip_ratio"):
        ring = t["rings"][name]
        lines.append("  `{}` {:+.1f} µs on {:.3f} ms ({:+.2f} %); {} chunks, {} record(s) per step; the bound clipped in {:.0f} % of the last {} steps "
                     "(smallest scale {:.3g}, {} bypassed).".format(name, 1e3 * (ms(t, name) - ms(t, "without_flags")), ms(t, "without_flags"),
                                                                     100 * (t["images_per_s"][name]["median"] / off["median"] - 1), ring["chunks"],
                                                                     ring["records_per_row"], 100 * ring["clip_frac"], ring["rows"], ring["scale_min"],
                                                                     ring["bypassed"]))
    lines.append("* **With `--inner-loop-log`** (the clip's ring read where the step ring is, once per meta-iteration), per step against `with_step_log`:")
    for name in ("clip_norm_log", "clip_ratio_log"):
        lines.append("  `{}` {:+.1f} µs on {:.3f} ms ({:+.2f} %).".format(name, 1e3 * (ms(t, name) - ms(t, "with_step_log")), ms(t, "with_step_log"),
                                                                          100 * (t["images_per_s"][name]["median"] / t["images_per_s"]["with_step_log"]["median"] - 1)))
    lines += ["* No target is set for the modes. NOT measured: the kernels' own times (no kernel trace was taken), EfficientNet-B3 at 384²,",
              "  larger meta-batches, concurrent lanes, Adam, evaluation fine-tunes, and a step with a non-finite gradient.", ""]
    with open(a.md, "w") as f:
        f.write("\n".join(lines))
    print("wrote {}".format(a.md))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds one repeat (and each learner's build + warm-up) may take")
    p.add_argument("--clip-norm", type=float, default=1.0, help="C of the clip_norm settings")
    p.add_argument("--clip-ratio", type=float, default=0.01, help="LAMBDA of the clip_ratio settings")
    p.add_argument("--clip-ratio-eps", type=float, default=1e-3)
    p.add_argument("--tree", default=None, help="checkout to import mliis_amd from (default: the one this file is in)")
    p.add_argument("--json", default=None)
    p.add_argument("--parent", default=None, help="built checkout of the parent commit: run it, this tree and it again in child processes")
    p.add_argument("--md", default=None, help="with --parent: the markdown file the table goes to")
    a = p.parse_args(argv)
    if a.parent:
        if not a.md:
            p.error("--parent needs --md")
        orchestrate(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
