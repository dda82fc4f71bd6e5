"""What flip test-time augmentation at evaluation costs, on one MI355X, default model (EfficientLab-6-3 on EfficientNet-B0, 224x224, fp32,
SGD):
  batch        per evaluation batch of 5 images (the transductive batch) and of 11 (a per-sample batch: 10 train images + 1 test image), the
               wall time of Learner.score_resident without views (views=(): the launches of the parent commit), with ("hflip",) and with all
               three views;
  op           the pair ops.view_gather (n images of 224 x 224 x 3 through an index vector, mirrored) + ops.view_merge (n maps of 56 x 56 x 2,
               mirrored back) alone, by device events around --op-launches pairs.
The expectation to confirm or refute: one forward pass per extra view plus two launches bound by their issue.
One GPU process per tree; the settings of a part alternate and each is timed --repeats times; host clock around calls that end in a device
synchronise.  Every repeat runs under its own time limit (SIGALRM with the default action: a repeat that exceeds --limit seconds ends the
process instead of hanging it).

    python tools/bench_tta.py [--iters 30] [--repeats 3] [--limit 120] [--tree DIR] [--json out.json]
    python tools/bench_tta.py --parent DIR --md profiles/tta.md [...]

--tree DIR imports mliis_amd from another checkout (the same tool on the parent commit: what it lacks is not timed).  --parent DIR (a built
checkout of the parent commit) makes this process an orchestrator that never touches the GPU itself: it starts one fresh child process
after the other -- the parent commit, this tree, the parent commit again -- stops at the first that fails, and writes the table of --md.
There is no CPU path: without a GPU this fails."""
import argparse
import inspect
import json
import os
import signal
import statistics
import subprocess
import sys
import time

VIEW_SETS = {"views_off": (), "hflip": ("hflip",), "all_three": ("hflip", "vflip", "hvflip")}


def _stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), repeats=v)


def measure(a):
    import torch
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta needs an MI355X: there is no CPU path and no number without one")
    import mliis_amd
    from mliis_amd import ops
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import synthetic_task
    assert os.path.dirname(os.path.abspath(mliis_amd.__file__)) == os.path.join(root, "mliis_amd"), mliis_amd.__file__
    dev = torch.device("cuda", 0)
    size = 224
    has_views = "views" in inspect.signature(Learner.score_resident).parameters

    def limited(fn):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(a.limit)
        try:
            return fn()
        finally:
            signal.alarm(0)

    def alternate(settings, n_calls):
        """{name: [ms per call, one per repeat]}: the settings alternate inside every repeat."""
        for fn in settings.values():
            limited(lambda: (fn(), fn(), torch.cuda.synchronize()))
        values = {k: [] for k in settings}
        for _ in range(a.repeats):
            for name, fn in settings.items():
                def timed():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(n_calls):
                        fn()
                    torch.cuda.synchronize()
                    return 1e3 * (time.perf_counter() - t0) / n_calls
                values[name].append(limited(timed))
        return {k: _stat(v) for k, v in values.items()}

    out = dict(tree=root, device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats, op_launches=a.op_launches)
    L = limited(lambda: Learner(image_size=size, rsd=(2, 4), learning_rate=1e-3, optimizer="sgd", seed=0, device=dev, max_shots=16))
    x, y = synthetic_task(16, size, seed=0)
    L.load_task(x, y)
    L.inner_step([0, 1, 2, 3, 4])
    out["batch_ms"], out["counts"] = {}, {}
    for n in (5, 11):
        idx = list(range(n))
        if has_views:
            settings = {k: (lambda v=v: L.score_resident(idx, views=v)) for k, v in VIEW_SETS.items()}
        else:
            settings = {"views_off": lambda: L.score_resident(idx)}
        out["batch_ms"][str(n)] = alternate(settings, a.iters)
        out["counts"][str(n)] = {k: fn().tolist() for k, fn in settings.items()}      # (the parent's and this tree's views_off rows must agree)
    L.close()
    if hasattr(ops, "view_gather"):
        out["op_us"] = {}
        for n in (5, 11):
            g = torch.Generator().manual_seed(n)
            pool = (torch.rand(16, size, size, 3, generator=g) * 255.0).to(dev)
            idx = torch.arange(n, dtype=torch.int32, device=dev)
            batch = torch.empty(n, size, size, 3, device=dev)
            small, acc = torch.randn(n, 56, 56, 2, generator=g).to(dev), torch.empty(n, 56, 56, 2, device=dev)

            def pair():
                ops.view_gather(pool, idx, "hflip", out=batch)
                ops.view_merge(acc, None, small, "hflip", 1.0)
            pair()
            torch.cuda.synchronize()
            vals = []
            for _ in range(a.repeats):
                def timed():
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for _ in range(a.op_launches):
                        pair()
                    e.record()
                    torch.cuda.synchronize()
                    return 1e3 * s.elapsed_time(e) / a.op_launches
                vals.append(limited(timed))
            out["op_us"][str(n)] = dict(_stat(vals), bytes=2 * 4 * (batch.numel() + small.numel()))
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


def _cell(d):
    return "-" if d is None else "{:.3f} ({:.3f}-{:.3f})".format(d["median"], d["min"], d["max"])


def _verdict(x, lo, hi):
    return "inside the spread" if lo <= x <= hi else "OUTSIDE the spread"


def orchestrate(a):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parent = os.path.abspath(a.parent)
    out_dir = os.path.dirname(os.path.abspath(a.md))
    os.makedirs(out_dir, exist_ok=True)
    runs = []
    for label, tree in (("parent commit, process 1", parent), ("this tree", here), ("parent commit, process 2", parent)):
        path = os.path.join(out_dir, ".bench_tta_{}.json".format(len(runs)))
        cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--repeats", str(a.repeats), "--limit", str(a.limit),
               "--op-launches", str(a.op_launches), "--tree", tree, "--json", path]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit * 40)
        if r.returncode != 0:      # nothing more is started on the device after a process that failed
            raise SystemExit("{} failed ({}):\n{}".format(label, r.returncode, r.stderr[-3000:]))
        with open(path) as f:
            runs.append((label, json.loads(f.read())))
        os.remove(path)
        print("{}: done".format(label), flush=True)
    p1, t, p2 = runs[0][1], runs[1][1], runs[2][1]
    L = ["# What flip test-time augmentation at evaluation costs", "",
         "One MI355X, `tools/bench_tta.py`: EfficientLab-6-3 on EfficientNet-B0, 224², fp32, SGD; `Learner.score_resident` of 5 images (the",
         "transductive batch) and of 11 (a per-sample batch). Host clock around calls that end in a device synchronise; every setting {} times,".format(t["repeats"]),
         "the settings alternating; median (min-max). Three processes, one after the other: the parent commit, this tree, the parent commit",
         "again (the parent has no views: its `score_resident` runs).", "",
         "    python tools/bench_tta.py --parent <built checkout of the parent commit> --md profiles/tta.md --iters {} --repeats {}".format(t["iters"], t["repeats"]), "",
         "## Per evaluation batch (ms per `score_resident` call, {} calls per repeat)".format(t["iters"]), "",
         "| images | views | this tree | parent, process 1 | parent, process 2 |", "|---|---|---|---|---|"]
    for n in ("5", "11"):
        for name in VIEW_SETS:
            L.append("| {} | `{}` | {} | {} | {} |".format(n, name, _cell(t["batch_ms"][n].get(name)), _cell(p1["batch_ms"][n].get(name)),
                                                        _cell(p2["batch_ms"][n].get(name))))
    L.append("")
    for n in ("5", "11"):
        b = t["batch_ms"][n]
        off, one, three = b["views_off"], b["hflip"], b["all_three"]
        a1, a2 = p1["batch_ms"][n]["views_off"], p2["batch_ms"][n]["views_off"]
        lo, hi = min(a1["min"], a2["min"]), max(a1["max"], a2["max"])
        same = t["counts"][n]["views_off"] == p1["counts"][n]["views_off"] == p2["counts"][n]["views_off"]
        L.append("* **{} images, views off**: {:.3f} ms (median) against {:.3f}-{:.3f} over the two processes of the parent commit (medians {:.3f} and "
                 "{:.3f}): {}; the counts are {} the parent's.".format(n, off["median"], lo, hi, a1["median"], a2["median"],
                                                                       _verdict(off["median"], lo, hi), "exactly" if same else "NOT"))
        L.append("* **{} images, with views**: `hflip` {:+.3f} ms = {:.2f} of a views-off call; all three {:+.3f} ms = {:.2f} of a views-off call per "
                 "extra view (the call without views: {:.3f} ms).".format(n, one["median"] - off["median"], (one["median"] - off["median"]) / off["median"],
                                                                          three["median"] - off["median"],
                                                                          (three["median"] - off["median"]) / (3 * off["median"]), off["median"]))
    L += ["", "## The gather + merge pair alone (µs per pair: `ops.view_gather` of n images 224 x 224 x 3 through an index vector and",
          "`ops.view_merge` of n maps 56 x 56 x 2, both mirrored; device events around {} pairs)".format(t["op_launches"]), "",
          "| images | this tree | bytes read + written per pair | GB/s at the median |", "|---|---|---|---|"]
    for n, v in t["op_us"].items():
        L.append("| {} | {} | {} | {:.0f} |".format(n, _cell(v), v["bytes"], v["bytes"] / v["median"] / 1e3))
    L += ["", "* The expectation was one forward pass per extra view plus two launches bound by their issue. A views-off call is one forward pass,",
          "  the counts launch and the 16-bytes-per-image copy back, so the ratios above are in units of slightly more than a forward pass; the",
          "  pair's own time is the table above. The figures confirm or refute it as they stand; no target is set.",
          "* NOT measured: the kernels' own times (no kernel trace was taken: the pair's figure is launch-to-launch time of two launches on an",
          "  otherwise idle stream), EfficientNet-B3 at 384², concurrent lanes, `mask_resident` / `histogram_resident` / `predict` with views,",
          "  and a whole `run_metasegnet.py` run. Nothing is claimed about IoU: there is no dataset here.", ""]
    with open(a.md, "w") as f:
        f.write("\n".join(L))
    print("wrote {}".format(a.md))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--iters", type=int, default=30, help="calls per repeat of the per-batch part")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--op-launches", type=int, default=200)
    p.add_argument("--limit", type=int, default=120, help="seconds one repeat (and the learner's build) may take")
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
