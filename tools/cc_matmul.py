"""cc_matmul against the forms it replaces, in one process on one GPU:
    python tools/cc_matmul.py [--presets silver,gold] [--shapes 2x2x2,4x4x4,1x8x4,4x8x1,4x2x4] [--min-seconds 0.3] [--rounds 3]
For every preset at level 0 and every shape m x k x n, over m k + k n distinct synthetic ciphertexts:
    matmul   cc_matmul(A, B): ONE native call (lf_cc_matmul)
    batch    cc_dot_batch over the same m n dots of k pairs
    loop     [cc_dot(pairs) for pairs in dots]
The forms of a point are timed alternately with device events after a warm-up of each, every timing over at least --min-seconds
of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its rounds) is
reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratios batch / matmul and
loop / matmul, and `faster`: whether matmul beats batch by more than the larger of the two spreads.
    python tools/cc_matmul.py --trace gold:4x4x4 [--calls 10] [--form matmul|batch|loop]
runs only that form of the point (for a kernel trace taken from outside, the program in a process of its own).
Synthetic keys and ciphertexts (utils/synth.py): the kernels do not look at the values."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")

from tools.hoisted_rotations import timed   # noqa: E402


def measure(forms, min_seconds, rounds):
    for fn in forms.values():
        fn()
    times = {f: [] for f in forms}
    for _ in range(rounds):
        for f, fn in forms.items():
            times[f].append(timed(fn, min_seconds))
    med = {f: statistics.median(t) for f, t in times.items()}
    spread = {f: (max(t) - min(t)) / med[f] for f, t in times.items()}
    out = {f: round(med[f], 1) for f in forms}
    out.update({f"spread_{f}": round(spread[f], 4) for f in forms})
    out["batch_over_matmul"] = round(med["batch"] / med["matmul"], 3)
    out["loop_over_matmul"] = round(med["loop"] / med["matmul"], 3)
    out["faster"] = bool(med["batch"] - med["matmul"] > max(spread["batch"] * med["batch"], spread["matmul"] * med["matmul"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--shapes", default="2x2x2,4x4x4,1x8x4,4x8x1,4x2x4")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", default=None, help="preset:MxKxN — run one form of that point alone, --calls times")
    ap.add_argument("--form", default="matmul", choices=("matmul", "batch", "loop"))
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cc_matmul: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    names = args.presets.split(",")
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    if args.trace:
        name, shape = args.trace.split(":")
        names, shapes = [name], [tuple(int(x) for x in shape.split("x"))]
    result = {"unit": "us per call (level 0)", "cc_matmul": []}
    for name in names:
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        assert eng._native_level(0) is not None and eng._native_level(1) is not None
        evk = synth.key_switch_key(eng, 77)
        for m, k, n in shapes:
            cts = [synth.ciphertext(eng, 50 + i, 0) for i in range(m * k + k * n)]
            A = [[cts[i * k + t] for t in range(k)] for i in range(m)]
            B = [[cts[m * k + t * n + j] for j in range(n)] for t in range(k)]
            dots = [[(A[i][t], B[t][j]) for t in range(k)] for i in range(m) for j in range(n)]
            calls = []
            real = eng.backend.cc_matmul_native
            eng.backend.cc_matmul_native = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
            eng.cc_matmul(A, B, evk)
            del eng.backend.cc_matmul_native
            assert calls == [1], "cc_matmul did not take its one native call"
            forms = {"matmul": lambda: eng.cc_matmul(A, B, evk), "batch": lambda: eng.cc_dot_batch(dots, evk),
                     "loop": lambda: [eng.cc_dot(pairs, evk) for pairs in dots]}
            if args.trace:
                for _ in range(args.calls):
                    forms[args.form]()
                torch.cuda.synchronize()
                continue
            point = {"preset": name, "m": m, "k": k, "n": n, **measure(forms, args.min_seconds, args.rounds)}
            result["cc_matmul"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
            del cts, A, B, dots
        del eng, evk
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
