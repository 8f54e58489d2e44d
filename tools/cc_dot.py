"""cc_dot against the two ways to write a sum of ciphertext products without it, in one process on one GPU:
    python tools/cc_dot.py [--presets silver,gold] [--ks 2,4,8,16] [--min-seconds 0.5] [--rounds 5]
For every (preset, k) at level 0, k pairs over four ciphertexts:
    dot      cc_dot(pairs)                                   one relinearisation for the sum
    mult     k x cc_mult, then the cc_add chain              (a)
    batch    cc_mult_batch(pairs), then the cc_add chain     (b)
The three forms are timed alternately with device events after a warm-up of each, every timing over at least --min-seconds of
work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its rounds) is
reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, and the ratios mult / dot and
batch / dot.  cc_dot "pays for itself" at a point when batch - dot exceeds batch's own spread there.
    python tools/cc_dot.py --trace gold:8 [--calls 10] [--form dot|mult|batch]
runs only that form at that point (for a kernel trace taken from outside, the program in a process of its own).
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

SLOTS = ((0, 1), (1, 0), (0, 0), (2, 3), (3, 1), (2, 2), (1, 3), (3, 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--ks", default="2,4,8,16")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", default=None, help="preset:k — run one form alone, --calls times")
    ap.add_argument("--form", default="dot", choices=("dot", "mult", "batch"))
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("cc_dot: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    names, ks = args.presets.split(","), [int(k) for k in args.ks.split(",")]
    if args.trace:
        names, ks = [args.trace.split(":")[0]], [int(args.trace.split(":")[1])]
    result = {"unit": "us per call (sum of k ciphertext products, level 0)", "points": []}
    for name in names:
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        assert eng._native_level(0) is not None and eng._native_level(1) is not None
        evk = synth.key_switch_key(eng, 77)
        cts = [synth.ciphertext(eng, 50 + i, 0) for i in range(4)]
        for k in ks:
            pairs = [(cts[i], cts[j]) for i, j in (SLOTS * (k // len(SLOTS) + 1))[:k]]

            def chain(products):
                acc = products[0]
                for p in products[1:]:
                    acc = eng.cc_add(acc, p)
                return acc

            forms = {"dot": lambda: eng.cc_dot(pairs, evk),
                     "mult": lambda: chain([eng.cc_mult(a, b, evk) for a, b in pairs]),
                     "batch": lambda: chain(eng.cc_mult_batch(pairs, evk))}
            if args.trace:
                for _ in range(args.calls):
                    forms[args.form]()
                torch.cuda.synchronize()
                continue
            for fn in forms.values():
                fn()
            times = {f: [] for f in forms}
            for _ in range(args.rounds):
                for f, fn in forms.items():
                    times[f].append(timed(fn, args.min_seconds))
            med = {f: statistics.median(t) for f, t in times.items()}
            spread = {f: (max(t) - min(t)) / med[f] for f, t in times.items()}
            point = {"preset": name, "k": k, **{f: round(med[f], 1) for f in forms},
                     **{f"spread_{f}": round(spread[f], 4) for f in forms},
                     "mult_over_dot": round(med["mult"] / med["dot"], 3), "batch_over_dot": round(med["batch"] / med["dot"], 3),
                     "pays": bool(med["batch"] - med["dot"] > max(times["batch"]) - min(times["batch"]))}
            result["points"].append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
        del eng, evk, cts
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
