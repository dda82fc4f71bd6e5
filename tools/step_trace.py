"""The launch sequence of the inner step as a hash: every C-ABI call (`lib.trace`) of an eager step, the capturing step, a replayed
step, a tail batch of 5 and predict() in both modes, per learner configuration, canonicalised so that two source trees that issue the
same launches with the same arguments print the same line.  Pointer arguments become `null`, `out` (a by-reference result) or the
index of that address's first appearance in the trace (aliasing, not addresses); every other argument keeps its exact value.
    python tools/step_trace.py [--only NAME ...] [--dump DIR]
Uses only Learner's public interface and imports the tree it lies in: copy the file into another checkout to compare the two."""
import argparse
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mliis_amd._lib import SIGNATURES, lib  # noqa: E402
from mliis_amd.learner import Learner  # noqa: E402
from mliis_amd.metaseg import synthetic_task  # noqa: E402

# name -> (image size, Learner keywords); the first seven are tests/test_step_poisoned_gpu.py::CONFIGS
CONFIGS = {
    "defaults": (64, dict()),
    "op_by_op_dice": (64, dict(small_fused=False, dw_march=False, dice=True, label_smoothing=0.1)),
    "darc1_adam": (64, dict(darc1=True, optimizer="adam")),
    "aspp": (64, dict(spatial_pyramid_pooling=True, skip_decoding=True)),
    "bf16_storage": (64, dict(matmul_precision="bf16-storage")),
    "full_224": (224, dict(matmul_precision="fp32")),
    "graph_fomaml_tail": (64, dict()),
    "fuse_bn2": (64, dict(fuse_bn2=True)),
    "fuse_bn2_224": (224, dict(fuse_bn2=True)),
    "no_fuse_head": (64, dict(fuse_head=False)),
    "fp32_native_224": (224, dict(matmul_precision="fp32-native")),
    "bf16_224": (224, dict(matmul_precision="bf16")),
    "fp8_224": (224, dict(matmul_precision="fp8")),
    "bf16_storage_224": (224, dict(matmul_precision="bf16-storage")),
    "b3_224": (224, dict(feature_extractor_name="efficientnet-b3")),
    "b3_bf16_storage_224": (224, dict(feature_extractor_name="efficientnet-b3", matmul_precision="bf16-storage")),
    "b3_op_by_op": (64, dict(feature_extractor_name="efficientnet-b3", small_fused=False, dw_march=False)),
    "dropout": (64, dict(final_layer_dropout_rate=0.5)),
    "no_drop_connect": (64, dict(drop_connect=False)),
    "aspp_only_adam_224": (224, dict(spatial_pyramid_pooling=True, optimizer="adam")),
    "no_rsd": (64, dict(rsd=[])),
}
_POINTERS = (C.c_void_p, C.c_char_p)


def canonical(calls):
    """One line per call: the entry point and its arguments, pointers replaced as the module docstring says."""
    seen, lines = {}, []
    for name, args in calls:
        if isinstance(name, int):   # (phase marker)
            lines.append("# " + args)
            continue
        out = []
        for t, v in zip(SIGNATURES[name][1], args):
            if t in _POINTERS or hasattr(t, "contents"):
                v = v.value if isinstance(v, C.c_void_p) else v
                if v is None or v == 0:
                    out.append("null")
                elif not isinstance(v, int):   # ctypes.byref(...)
                    out.append("out")
                else:
                    out.append("p%d" % seen.setdefault(v, len(seen)))
            else:
                out.append(repr(v))
        lines.append("{}({})".format(name, ", ".join(out)))
    return "\n".join(lines) + "\n"


def trace(H, kw):
    L = Learner(image_size=H, use_graph=True, seed=3, **kw)
    try:
        x, y = synthetic_task(10, H, seed=2)
        L.load_task(x, y)
        lib.trace = calls = []
        for phase, idx in (("eager", [0, 1, 2, 3, 4, 5, 6, 7]), ("capture", [7, 6, 5, 4, 3, 2, 1, 0]), ("replay", [1, 3, 5, 7, 9, 0, 2, 4]),
                           ("tail", [9, 8, 7, 6, 5])):
            calls.append((0, phase))
            L.inner_step(idx)
        for training in (False, True):
            calls.append((0, "predict training={}".format(training)))
            L.predict(x[:3], training=training)
        L.synchronize()
    finally:
        lib.trace = None
        L.close()
    return calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None, help="configuration names (default: all)")
    ap.add_argument("--dump", default=None, help="directory that receives the canonical text of every configuration")
    a = ap.parse_args()
    for name in a.only or CONFIGS:
        H, kw = CONFIGS[name]
        calls = trace(H, kw)
        text = canonical(calls)
        if a.dump:
            os.makedirs(a.dump, exist_ok=True)
            with open(os.path.join(a.dump, name + ".txt"), "w") as f:
                f.write(text)
        print("%-22s %6d calls  %s" % (name, sum(1 for n, _ in calls if not isinstance(n, int)), hashlib.sha256(text.encode()).hexdigest()), flush=True)


if __name__ == "__main__":
    main()
