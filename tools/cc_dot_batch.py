"""cc_dot_batch and poly_eval_batch against the loops they replace, in one process on one GPU:
    python tools/cc_dot_batch.py [--presets silver,gold] [--dots 4,8] [--pairs 2,8] [--cts 8] [--min-seconds 0.5] [--rounds 5]
For every preset at level 0:
    (a) per (B, k) of --dots x --pairs, B dots of k pairs each over four ciphertexts:
        batch    cc_dot_batch(dots)                      the key read once per group of 4 dots
        loop     [cc_dot(pairs) for pairs in dots]
    (b) per polynomial (degree 15 in the power basis, degree 31 in the Chebyshev basis on (-8, 8)), --cts ciphertexts:
        batch    poly_eval_batch(cts, coeffs)
        loop     [poly_eval(ct, coeffs) for ct in cts]
The two forms of a point are timed alternately with device events after a warm-up of each, every timing over at least
--min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its
rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads and the ratio loop / batch.
    python tools/cc_dot_batch.py --trace gold:4:8 [--calls 10] [--form batch|loop]
runs only that form of the cc_dot_batch point preset:B:k (for a kernel trace taken from outside, the program in a process of its
own).  Synthetic keys and ciphertexts (utils/synth.py): the kernels do not look at the values."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")

from tools.cc_dot import SLOTS              # noqa: E402
from tools.hoisted_rotations import timed   # noqa: E402


def measure(forms, min_seconds, rounds):
    for fn in forms.values():
        fn()
    times = {f: [] for f in forms}
    for _ in range(rounds):
        for f, fn in forms.items():
            times[f].append(timed(fn, min_seconds))
    med = {f: statistics.median(t) for f, t in times.items()}
    out = {f: round(med[f], 1) for f in forms}
    out.update({f"spread_{f}": round((max(t) - min(t)) / med[f], 4) for f, t in times.items()})
    out["loop_over_batch"] = round(med["loop"] / med["batch"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--pairs", default="2,8")
    ap.add_argument("--cts", type=int, default=8)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", default=None, help="preset:B:k — run one form of that cc_dot_batch point alone, --calls times")
    ap.add_argument("--form", default="batch", choices=("batch", "loop"))
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cc_dot_batch: no GPU")
    import numpy as np
    from numpy.polynomial import chebyshev as C
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    names = args.presets.split(",")
    shapes = [(int(b), int(k)) for b in args.dots.split(",") for k in args.pairs.split(",")]
    if args.trace:
        name, b, k = args.trace.split(":")
        names, shapes = [name], [(int(b), int(k))]
    polys = [("power", np.random.default_rng(5).uniform(-1, 1, 16), None),
             ("chebyshev", C.chebinterpolate(lambda t: 1.0 / (1.0 + np.exp(-8.0 * t)), 31), (-8, 8))]
    result = {"unit": "us per call (level 0)", "cc_dot_batch": [], "poly_eval_batch": []}
    for name in names:
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        assert eng._native_level(0) is not None and eng._native_level(1) is not None
        evk = synth.key_switch_key(eng, 77)
        cts = [synth.ciphertext(eng, 50 + i, 0) for i in range(4)]
        for B, k in shapes:
            slots = SLOTS * (B + k)
            dots = [[(cts[i], cts[j]) for i, j in slots[d:d + k]] for d in range(B)]
            forms = {"batch": lambda: eng.cc_dot_batch(dots, evk), "loop": lambda: [eng.cc_dot(pairs, evk) for pairs in dots]}
            if args.trace:
                for _ in range(args.calls):
                    forms[args.form]()
                torch.cuda.synchronize()
                continue
            point = {"preset": name, "dots": B, "pairs": k, **measure(forms, args.min_seconds, args.rounds)}
            result["cc_dot_batch"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
        if not args.trace:
            xs = [synth.ciphertext(eng, 60 + i, 0) for i in range(args.cts)]
            for basis, coeffs, interval in polys:
                degree = len(coeffs) - 1
                assert eng.poly_depth(degree, basis, interval) < eng.num_levels
                forms = {"batch": lambda: eng.poly_eval_batch(xs, coeffs, evk, basis=basis, interval=interval),
                         "loop": lambda: [eng.poly_eval(x, coeffs, evk, basis=basis, interval=interval) for x in xs]}
                point = {"preset": name, "cts": args.cts, "basis": basis, "degree": degree,
                         **measure(forms, args.min_seconds, args.rounds)}
                point["loop_per_ct"] = round(point["loop"] / args.cts, 1)     # one poly_eval
                result["poly_eval_batch"].append(point)
                print(json.dumps(point), file=sys.stderr, flush=True)
            del xs
        del eng, evk, cts
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
