"""What the Tversky region term costs, and what its three-launch head saves against the dice chain: inner-loop images/s at config 2 of
BASELINE.json (EfficientLab-6-3, 224x224, meta-batch 1, 5 shots, 8 inner steps of batch 8, fp32, SGD, one MI355X)
  without_flags      Learner() and Gecko() as always: the fused head with its fold riding in the final conv's backward-data launch;
  bce_dice           --loss_name bce_dice: Learner(dice=True) -- the unchanged chain resize -> partial sums -> fold -> gradient -> resize^T
                     over full-resolution tensors (the yardstick);
  tversky_1_1        --tversky 1 1: the same loss on mliis_head_tversky_fused (csrc/tversky.hip): sums, fold, gradient tiles on the
                     decoder's map;
  tversky            --tversky A B;
  tversky_focal      --tversky A B --focal-gamma G --fg-weight W.
One GPU process per tree, the learners built once; every setting is timed --repeats times, the settings alternating so that drift falls on
all; host clock around --steps meta-steps that end in a device synchronise, after --warmup untimed ones.  Every repeat runs under its own
time limit (SIGALRM with the default action: a repeat that exceeds --limit seconds ends the process instead of hanging it).

    python tools/bench_tversky.py [--steps 100] [--warmup 5] [--repeats 3] [--limit 120] [--tree DIR] [--json out.json]
    python tools/bench_tversky.py --parent DIR --md profiles/tversky.md [--title "..."] [...]

--tree DIR imports mliis_amd from another checkout (the same tool on the parent commit: a Learner that does not know `tversky` is timed in
the settings it has).  --parent DIR (a built checkout of the parent commit) makes this process an orchestrator that never touches the GPU
itself: it starts one fresh child process after the other -- the parent commit, this tree, the parent commit again -- stops at the first
that fails, and writes the table of --md from their results, keeping what the file holds below the line MANUAL_MARK.  There is no CPU path:
without a GPU this fails."""
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

SETTINGS = ("without_flags", "bce_dice", "tversky_1_1", "tversky", "tversky_focal")
MANUAL_MARK = "<!-- below this line: written by hand, kept by tools/bench_tversky.py -->"


def measure(a):
    import torch
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tversky needs an MI355X: there is no CPU path and no number without one")
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

    def build(learner_kw):
        L = Learner(image_size=size, rsd=(2, 4), learning_rate=1e-3, optimizer="sgd", seed=0, device=dev, max_shots=16, **learner_kw)
        with contextlib.redirect_stdout(io.StringIO()):
            meta = Gecko(L, rng_mode="per_task", seed=0)
        return L, meta

    def meta_steps(meta, n):
        for _ in range(n):
            meta.train_step(tasks, num_shots=shots, inner_batch_size=inner_batch, inner_iters=inner_iters, replacement=False, meta_step_size=0.1,
                            meta_batch_size=1)

    pair = (a.alpha, a.beta)
    wanted = dict(without_flags={}, bce_dice=dict(dice=True), tversky_1_1=dict(tversky=(1.0, 1.0)), tversky=dict(tversky=pair),
                  tversky_focal=dict(tversky=pair, focal_gamma=a.gamma, fg_weight=a.fg_weight))
    settings = {}
    for name in SETTINGS:
        try:
            settings[name] = limited(lambda: build(wanted[name]))
        except TypeError as e:       # a checkout from before the option
            print("this checkout has no {} setting ({}): not timed".format(name, e), file=sys.stderr)
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
    losses = {k: L.loss_value() for k, (L, _) in settings.items()}
    out = dict(config="BASELINE.json configs[1]: 224x224, meta-batch 1, 5-shot x 8 inner steps of batch 8, fp32, SGD, 1 GPU", unit="images/s",
               steps=a.steps, warmup=a.warmup, repeats=a.repeats, tree=root, device=torch.cuda.get_device_name(0), alpha=a.alpha, beta=a.beta,
               gamma=a.gamma, fg_weight=a.fg_weight, images_per_step=inner_batch, last_loss=losses,
               images_per_s={k: dict(median=statistics.median(v), min=min(v), max=max(v), repeats=v) for k, v in values.items()})
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
        path = os.path.join(out_dir, ".bench_tversky_{}.json".format(len(runs)))
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats),
               "--limit", str(a.limit), "--alpha", str(a.alpha), "--beta", str(a.beta), "--gamma", str(a.gamma), "--fg-weight", str(a.fg_weight),
               "--tree", tree, "--json", path]
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
    flags = {"without_flags": "(none)", "bce_dice": "`--loss_name bce_dice`", "tversky_1_1": "`--tversky 1 1`",
             "tversky": "`--tversky {} {}`".format(t["alpha"], t["beta"]),
             "tversky_focal": "`--tversky {} {} --focal-gamma {} --fg-weight {}`".format(t["alpha"], t["beta"], t["gamma"], t["fg_weight"])}
    lines = ["# " + a.title, "",
             "One MI355X, `tools/bench_tversky.py`: config 2 of `BASELINE.json` (EfficientLab-6-3, 224², meta-batch 1, 5 shots, 8 inner SGD steps of",
             "batch 8, fp32, captured graphs), inner-loop images/s of `Gecko.train_step`. Host clock around {} meta-steps that end in a device".format(t["steps"]),
             "synchronise, after {} untimed ones; every setting {} times, the settings alternating. Three processes, one after the other: the".format(t["warmup"], t["repeats"]),
             "parent commit, this tree, the parent commit again (the parent commit has no `--tversky`).", "",
             "    python tools/bench_tversky.py --parent <built checkout of the parent commit> --md {} --steps {} --warmup {} --repeats {}".format(
                 os.path.relpath(os.path.abspath(a.md), here), t["steps"], t["warmup"], t["repeats"]), "",
             "| setting | flags | this tree: median (min-max) images/s | parent, process 1 | parent, process 2 |", "|---|---|---|---|---|"]
    for name in SETTINGS:
        lines.append("| `{}` | {} | {} | {} | {} |".format(name, flags[name], _cell(t, name), _cell(p1, name), _cell(p2, name)))
    lines.append("")
    for name, title in (("without_flags", "Flags off"), ("bce_dice", "`--loss_name bce_dice` (the unchanged five-launch chain)")):
        off, a1, a2 = t["images_per_s"][name], p1["images_per_s"][name], p2["images_per_s"][name]
        lo, hi = min(a1["min"], a2["min"]), max(a1["max"], a2["max"])
        inside = lo <= off["median"] <= hi
        lines += ["* **{}**: {:.1f} images/s (median) against {:.1f}-{:.1f} over the two processes of the parent commit (medians {:.1f} and {:.1f}): {}.".format(
            title, off["median"], lo, hi, a1["median"], a2["median"],
            "inside the spread between the two" if inside else "OUTSIDE the spread between the two ({:+.2f} % against their mean)".format(
                100 * (off["median"] / ((a1["median"] + a2["median"]) / 2) - 1)))]
    base = (ms(p1, "bce_dice") + ms(p2, "bce_dice")) / 2
    lines += ["* Per 8-image inner step against `bce_dice` of the parent commit ({:.3f} ms, the mean of its two processes' medians; the two lie".format(base),
              "  {:.1f} µs apart):".format(1e3 * abs(ms(p1, "bce_dice") - ms(p2, "bce_dice")))]
    for name in ("bce_dice", "tversky_1_1", "tversky", "tversky_focal", "without_flags"):
        lines.append("  * `{}` of this tree: {:.3f} ms, {:+.1f} µs ({:+.2f} %)".format(name, ms(t, name), 1e3 * (ms(t, name) - base),
                                                                                  100 * (ms(t, name) / base - 1)))
    lines += ["* NOT measured: the kernels' own times (no kernel trace was taken), EfficientNet-B3 at 384², larger meta-batches, concurrent lanes,",
              "  Adam, the DARC1 / `fuse_head=False` chain (`mliis_tversky_ce`), and any effect on IoU (that needs a dataset).  No target is set, and",
              "  whether `--loss_name bce_dice` should be routed to the new head is left to another change.", ""]
    manual = ""
    if os.path.exists(a.md):
        old = open(a.md).read()
        if MANUAL_MARK in old:
            manual = old[old.index(MANUAL_MARK):]
    with open(a.md, "w") as f:
        f.write("\n".join(lines) + ("\n" + manual if manual else ""))
    print("wrote {}".format(a.md))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--limit", type=int, default=120, help="seconds one repeat (and each learner's build + warm-up) may take")
    p.add_argument("--alpha", type=float, default=0.3, help="ALPHA of the tversky settings")
    p.add_argument("--beta", type=float, default=0.7, help="BETA of the tversky settings")
    p.add_argument("--gamma", type=float, default=2.0, help="G of the tversky_focal setting")
    p.add_argument("--fg-weight", type=float, default=4.0, help="W of the tversky_focal setting")
    p.add_argument("--tree", default=None, help="checkout to import mliis_amd from (default: the one this file is in)")
    p.add_argument("--json", default=None)
    p.add_argument("--parent", default=None, help="built checkout of the parent commit: run it, this tree and it again in child processes")
    p.add_argument("--md", default=None, help="with --parent: the markdown file the table goes to")
    p.add_argument("--title", default="What the Tversky region term costs, and its head against the dice chain", help="with --md: the file's heading")
    a = p.parse_args(argv)
    if a.parent:
        if not a.md:
            p.error("--parent needs --md")
        orchestrate(a)
    else:
        measure(a)


if __name__ == "__main__":
    main()
