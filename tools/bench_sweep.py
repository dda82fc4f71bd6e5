"""What the evaluation threshold sweep costs, on one MI355X, default model (EfficientLab-6-3 on EfficientNet-B0, 224x224, fp32, SGD):
  batch        per evaluation batch of 5 images (the transductive batch) and of 11 (a per-sample batch: 10 train images + 1 test image), the
               wall time of Learner.score_resident (--device-metrics), of Learner.histogram_resident (--threshold-sweep: the same forward
               pass, the histogram launch instead of the counts launch, 2 KB per image back instead of 16 bytes), and of what a user does
               without it: predict(..., return_logits=True), softmax and a 2 x 256 numpy histogram on the host;
  pass         one final evaluation pass (Gecko.evaluate over --tasks synthetic tasks, 5 shots, 4 fine-tune steps of batch 5, 5 test images
               per task, per-sample predictions) with device_metrics alone and with the threshold_sweep sink;
  op           ops.prob_histogram alone on decoder logits N(0, 3) (unsaturated) and N(0, 8) (saturated: bins 0 and 255 hold almost half of the
               pixels), 5 and 11 images and -- the two launches of a real batch are bound by their issue -- 64, by device events around
               --op-launches launches.  With --sweep-lib PATH the library is another build of
               csrc/sweep.hip (MLIIS_SWEEP_LIB): how the kernel with the ballot split of bins 0 / 255 was measured.
One GPU process per tree; the settings of a part alternate and each is timed --repeats times; host clock around calls that end in a
device synchronise.  Every repeat runs under its own time limit (SIGALRM with the default action: a repeat that exceeds --limit seconds
ends the process instead of hanging it).

    python tools/bench_sweep.py [--iters 30] [--repeats 3] [--tasks 4] [--limit 120] [--tree DIR] [--sweep-lib PATH] [--json out.json]
    python tools/bench_sweep.py --parent DIR --md profiles/sweep.md [--ballot-lib PATH] [...]

--tree DIR imports mliis_amd from another checkout (the same tool on the parent commit: what it lacks is not timed).  --parent DIR (a built
checkout of the parent commit) makes this process an orchestrator that never touches the GPU itself: it starts one fresh child process
after the other -- the parent commit, this tree, (with --ballot-lib: this tree's op part on that library,) the parent commit again -- stops
at the first that fails, and writes the table of --md.  There is no CPU path: without a GPU this fails."""
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


def _stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), repeats=v)


def measure(a):
    if a.sweep_lib:
        os.environ["MLIIS_SWEEP_LIB"] = os.path.abspath(a.sweep_lib)
    import numpy as np
    import torch
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("bench_sweep needs an MI355X: there is no CPU path and no number without one")
    import mliis_amd
    from mliis_amd import ops
    from mliis_amd.learner import Learner
    from mliis_amd.metaseg import DeviceTask, synthetic_task
    from mliis_amd.reptile import Gecko
    assert os.path.dirname(os.path.abspath(mliis_amd.__file__)) == os.path.join(root, "mliis_amd"), mliis_amd.__file__
    dev = torch.device("cuda", 0)
    size = 224
    has_sweep = hasattr(Learner, "histogram_resident")

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

    out = dict(tree=root, device=torch.cuda.get_device_name(0), iters=a.iters, repeats=a.repeats, tasks=a.tasks, sweep_lib=a.sweep_lib,
               op_launches=a.op_launches)
    if not a.op_only:
        L = limited(lambda: Learner(image_size=size, rsd=(2, 4), learning_rate=1e-3, optimizer="sgd", seed=0, device=dev, max_shots=16))
        x, y = synthetic_task(16, size, seed=0)
        L.load_task(x, y)
        L.inner_step([0, 1, 2, 3, 4])
        xs = torch.from_numpy(x).to(dev)
        lab = np.rint(y[..., 1]) != 0

        def host_histogram(idx):
            _, logits = L.predict(xs[idx], return_logits=True)
            z = logits.cpu().numpy()
            p1 = 1.0 / (1.0 + np.exp(z[..., 0] - z[..., 1]))
            return [[np.histogram(p1[j][lab[i] == c], bins=256, range=(0.0, 1.0))[0] for c in (False, True)] for j, i in enumerate(idx)]

        out["batch_ms"] = {}
        for n in (5, 11):
            idx = list(range(n))
            settings = {"score_resident": lambda: L.score_resident(idx), "predict_logits_numpy": lambda: host_histogram(idx)}
            if has_sweep:
                settings["histogram_resident"] = lambda: L.histogram_resident(idx)
            out["batch_ms"][str(n)] = alternate(settings, a.iters)
        tasks = []
        for i in range(a.tasks):
            tx, ty = synthetic_task(10, size, seed=100 + i)
            tasks.append(DeviceTask("synthetic_%d" % i, torch.from_numpy(tx).to(dev), torch.from_numpy(ty).to(dev)))

        def one_pass(meta):
            with contextlib.redirect_stdout(io.StringIO()):
                meta.evaluate(list(tasks), num_shots=5, inner_batch_size=5, inner_iters=4, eval_all_tasks=True, test_shots=5)

        with contextlib.redirect_stdout(io.StringIO()):
            metas = {"device_metrics": Gecko(L, rng_mode="reference", device_metrics=True)}
            if has_sweep:
                from mliis_amd.metrics import ThresholdSweep
                metas["threshold_sweep"] = Gecko(L, rng_mode="reference", device_metrics=True, threshold_sweep=ThresholdSweep())
        out["pass_ms"] = alternate({k: (lambda m=m: one_pass(m)) for k, m in metas.items()}, 1)
        out["pass_images"] = a.tasks * 5
        L.close()
    if hasattr(ops, "prob_histogram"):
        out["op_us"] = {}
        for n in (5, 11, 64):
            for name, sd in (("unsaturated", 3.0), ("saturated", 8.0)):
                g = torch.Generator().manual_seed(n)
                small = (torch.randn(n, 56, 56, 2, generator=g) * sd).to(dev)
                l1 = (torch.rand(n, size, size, generator=g) < 0.3).float()
                labels = torch.stack([1.0 - l1, l1], dim=-1).contiguous().to(dev)
                hist = torch.zeros(n, 2, 256, dtype=torch.int32, device=dev)
                ops.prob_histogram(small, (size, size), labels, None, hist=hist)
                torch.cuda.synchronize()
                ends = float(hist[:, :, [0, 255]].sum()) / float(hist.sum())
                vals = []
                for _ in range(a.repeats):
                    def timed():
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        for _ in range(a.op_launches):
                            ops.prob_histogram(small, (size, size), labels, None, hist=hist)
                        e.record()
                        torch.cuda.synchronize()
                        return 1e3 * s.elapsed_time(e) / a.op_launches
                    vals.append(limited(timed))
                out["op_us"]["{}_{}".format(n, name)] = dict(_stat(vals), end_bin_share=ends)
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


def _cell(d, unit=""):
    return "-" if d is None else "{:.3f} ({:.3f}-{:.3f}){}".format(d["median"], d["min"], d["max"], unit)


def _verdict(x, lo, hi):
    return "inside the spread" if lo <= x <= hi else "OUTSIDE the spread"


def orchestrate(a):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    parent = os.path.abspath(a.parent)
    out_dir = os.path.dirname(os.path.abspath(a.md))
    os.makedirs(out_dir, exist_ok=True)
    plan = [("parent commit, process 1", parent, []), ("this tree", here, [])]
    if a.ballot_lib:
        plan.append(("this tree, op part, library with the ballot split", here, ["--op-only", "--sweep-lib", os.path.abspath(a.ballot_lib)]))
    plan.append(("parent commit, process 2", parent, []))
    runs = []
    for label, tree, extra in plan:
        path = os.path.join(out_dir, ".bench_sweep_{}.json".format(len(runs)))
        cmd = [sys.executable, os.path.abspath(__file__), "--iters", str(a.iters), "--repeats", str(a.repeats), "--tasks", str(a.tasks), "--limit",
               str(a.limit), "--op-launches", str(a.op_launches), "--tree", tree, "--json", path] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit * 40)
        if r.returncode != 0:      # nothing more is started on the device after a process that failed
            raise SystemExit("{} failed ({}):\n{}".format(label, r.returncode, r.stderr[-3000:]))
        with open(path) as f:
            runs.append((label, json.loads(f.read())))
        os.remove(path)
        print("{}: done".format(label), flush=True)
    p1, t, p2 = runs[0][1], runs[1][1], runs[-1][1]
    ballot = runs[2][1] if a.ballot_lib else None
    L = ["# What the evaluation threshold sweep costs", "",
         "One MI355X, `tools/bench_sweep.py`: EfficientLab-6-3 on EfficientNet-B0, 224², fp32, SGD. Host clock around calls that end in a device",
         "synchronise; every setting {} times, the settings of a part alternating; median (min-max). Separate processes, one after the other:".format(t["repeats"]),
         "the parent commit, this tree, the parent commit again (the parent has no sweep: its `score_resident`, host path and",
         "`device_metrics` pass run).", "",
         "    python tools/bench_sweep.py --parent <built checkout of the parent commit> --md profiles/sweep.md --iters {} --repeats {} --tasks {}{}".format(
             t["iters"], t["repeats"], t["tasks"], " --ballot-lib <library with the ballot split>" if ballot else ""), "",
         "## Per evaluation batch (ms per call, {} calls per repeat)".format(t["iters"]), "",
         "| images | call | this tree | parent, process 1 | parent, process 2 |", "|---|---|---|---|---|"]
    for n in ("5", "11"):
        for name in ("score_resident", "histogram_resident", "predict_logits_numpy"):
            L.append("| {} | `{}` | {} | {} | {} |".format(n, name, _cell(t["batch_ms"][n].get(name)), _cell(p1["batch_ms"][n].get(name)),
                                                          _cell(p2["batch_ms"][n].get(name))))
    L.append("")
    for n in ("5", "11"):
        b = t["batch_ms"][n]
        s, h, u = b["score_resident"], b["histogram_resident"], b["predict_logits_numpy"]
        lo, hi = min(s["min"], p1["batch_ms"][n]["score_resident"]["min"], p2["batch_ms"][n]["score_resident"]["min"]), \
            max(s["max"], p1["batch_ms"][n]["score_resident"]["max"], p2["batch_ms"][n]["score_resident"]["max"])
        L.append("* **{} images**: `histogram_resident` {:+.3f} ms against `score_resident` ({:.3f} against {:.3f}; `score_resident` spans {:.3f}-{:.3f} over "
                 "the three processes: the histogram's median is {}); the host path takes {:.1f} ms, {:.1f} times the histogram call.".format(
                     n, h["median"] - s["median"], h["median"], s["median"], lo, hi, _verdict(h["median"], lo, hi), u["median"], u["median"] / h["median"]))
    L += ["", "## One final evaluation pass (ms; {} tasks, 5 shots, 4 fine-tune steps of batch 5, 5 test images each, per-sample batches of 6)".format(t["tasks"]), "",
          "| setting | this tree | parent, process 1 | parent, process 2 |", "|---|---|---|---|"]
    for name in ("device_metrics", "threshold_sweep"):
        L.append("| `{}` | {} | {} | {} |".format(name, _cell(t["pass_ms"].get(name)), _cell(p1["pass_ms"].get(name)), _cell(p2["pass_ms"].get(name))))
    d, w = t["pass_ms"]["device_metrics"], t["pass_ms"]["threshold_sweep"]
    a1, a2 = p1["pass_ms"]["device_metrics"], p2["pass_ms"]["device_metrics"]
    lo, hi = min(a1["min"], a2["min"]), max(a1["max"], a2["max"])
    L += ["", "* **Without the flag**: {:.1f} ms (median) against {:.1f}-{:.1f} over the two processes of the parent commit (medians {:.1f} and {:.1f}): {}.".format(
        d["median"], lo, hi, a1["median"], a2["median"], _verdict(d["median"], lo, hi)),
        "* **With `--threshold-sweep`**: {:+.1f} ms on {:.1f} ms ({:+.2f} %); the repeats of `device_metrics` in this process span {:.1f}-{:.1f} ms: the "
        "sweep's median is {}.".format(w["median"] - d["median"], d["median"], 100 * (w["median"] / d["median"] - 1), d["min"], d["max"],
                                       _verdict(w["median"], d["min"], d["max"])),
        "", "## The histogram launches alone (µs per `ops.prob_histogram` call: the zeroing launch and the histogram launch; device events around {} calls)".format(
            t["op_launches"]), "",
        "| images | logits | pixels in bins 0 / 255 | every lane to the LDS atomics (shipped) | with the ballot split |", "|---|---|---|---|---|"]
    for key, v in t["op_us"].items():
        n, name = key.split("_")
        L.append("| {} | {} | {:.0f} % | {} | {} |".format(n, "N(0, 3), unsaturated" if name == "unsaturated" else "N(0, 8), saturated", 100 * v["end_bin_share"],
                                                         _cell(v), _cell(ballot["op_us"][key]) if ballot else "not measured"))
    L += ["", "* With the ballot split = the same kernel counting bins 0 and 255 of either class per wave with `__ballot` + `__popcll` and sending only",
          "  the other lanes to the LDS atomics, built out of tree for this measurement only (`MLIIS_SWEEP_LIB`); the results are identical either",
          "  way (integers). At 5 and 11 images the two launches are bound by their issue; at 64 images the kernel shows. The source keeps the",
          "  form that is not slower on the saturated logits, which is also the simpler one.",
          "* No target is set. NOT measured: the kernels' own times (no `rocprofv3 --kernel-trace --stats` run was taken; the figures above are",
          "  launch-to-launch times of two launches on an otherwise idle stream), EfficientNet-B3 at 384², concurrent lanes,",
          "  `--save-predictions` with the sweep, and a whole `run_metasegnet.py` run.", ""]
    with open(a.md, "w") as f:
        f.write("\n".join(L))
    print("wrote {}".format(a.md))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--iters", type=int, default=30, help="calls per repeat of the per-batch part")
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--tasks", type=int, default=4, help="tasks of the evaluation pass")
    p.add_argument("--op-launches", type=int, default=200)
    p.add_argument("--limit", type=int, default=120, help="seconds one repeat (and the learner's build) may take")
    p.add_argument("--tree", default=None, help="checkout to import mliis_amd from (default: the one this file is in)")
    p.add_argument("--sweep-lib", default=None, help="another build of libmliis_sweep.so to load (MLIIS_SWEEP_LIB)")
    p.add_argument("--op-only", action="store_true", help="only the op part")
    p.add_argument("--json", default=None)
    p.add_argument("--parent", default=None, help="built checkout of the parent commit: run it, this tree and it again in child processes")
    p.add_argument("--ballot-lib", default=None, help="with --parent: a library built with the ballot split of bins 0 / 255, for the op part")
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
