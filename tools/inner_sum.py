"""inner_sum and rotate_sum against the loops of existing ops they replace, in one process:
    python tools/inner_sum.py [--presets silver,gold] [--ns 16,64,0] [--radices 2,4,8] [--ks 3,7] [--min-seconds 0.5]
inner_sum(ct, n, radix) (n = 0 stands for num_slots) against the log fold   for k: ct = cc_add(rotate_single(ct, key[2^k]), ct)
and rotate_sum(ct, k keys) (with the self term) against   acc = ct; for r in rotate_hoisted(ct, keys): acc = cc_add(acc, r),
at level 0.  For every point the forms are timed alternately with device events after a warm-up, each over at least
--min-seconds of work, three rounds, the median kept.  Prints one JSON line: microseconds per call for each form and the ratio
(loop / new op).
    python tools/inner_sum.py --trace gold:64:4 [--calls 20]
runs only inner_sum at that preset:n:radix (for a kernel trace taken from outside, the program in a process of its own).
Synthetic keys and ciphertexts (utils/synth.py), one key per step: the kernels do not look at the values."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")

from tools.hoisted_rotations import timed   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--ns", default="16,64,0", help="block sizes, powers of two; 0 = num_slots")
    ap.add_argument("--radices", default="2,4,8")
    ap.add_argument("--ks", default="3,7", help="key counts of the rotate_sum points")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", default=None, help="preset:n:radix — run inner_sum alone, --calls times")
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("inner_sum: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, encdec, presets
    from liberate_fhe_amd.utils import synth
    names, ns = args.presets.split(","), [int(n) for n in args.ns.split(",") if n]
    radices, ks = [int(r) for r in args.radices.split(",")], [int(k) for k in args.ks.split(",") if k]
    if args.trace:
        name, n, radix = args.trace.split(":")
        names, ns, radices, ks = [name], [int(n)], [int(radix)], []
    result = {"unit": "us per call, level 0", "points": []}
    for name in names:
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        ct = synth.ciphertext(eng, 7, 0)
        keys = {}

        def key(step):
            if step not in keys:
                keys[step] = synth.key_switch_key(eng, 100 + len(keys), origin=f"rotation key:{step}")
            return keys[step]

        for n in ns:
            n = n or eng.num_slots
            fold_keys = [key(1 << k) for k in range(n.bit_length() - 1)]
            assert 1 << len(fold_keys) == n, "the log fold this tool compares against needs a power of two"

            def fold():
                x = ct
                for k in fold_keys:
                    x = eng.cc_add(eng.rotate_single(x, k), x)
                return x

            for radix in radices:
                rk = {s: key(s) for s in eng.inner_sum_steps(n, 1, radix)}
                new = lambda: eng.inner_sum(ct, n, rk, radix=radix)
                if args.trace:
                    for _ in range(args.calls):
                        new()
                    torch.cuda.synchronize()
                    continue
                fold(), new()
                t_old, t_new = [], []
                for _ in range(args.rounds):
                    t_old.append(timed(fold, args.min_seconds))
                    t_new.append(timed(new, args.min_seconds))
                a, b = statistics.median(t_old), statistics.median(t_new)
                result["points"].append({"preset": name, "op": "inner_sum", "n": n, "radix": radix, "keys": len(rk),
                                         "stages": [r for r, _ in encdec.inner_sum_plan(n, 1, eng.num_slots, radix)],
                                         "log_fold": round(a, 1), "inner_sum": round(b, 1), "ratio": round(a / b, 3)})
                print(json.dumps(result["points"][-1]), file=sys.stderr, flush=True)
        for k in ks:
            rks = [key(s) for s in range(1, k + 1)]

            def loop():
                acc = ct
                for r in eng.rotate_hoisted(ct, rks):
                    acc = eng.cc_add(acc, r)
                return acc

            new = lambda: eng.rotate_sum(ct, rks, include_self=True)
            loop(), new()
            t_old, t_new = [], []
            for _ in range(args.rounds):
                t_old.append(timed(loop, args.min_seconds))
                t_new.append(timed(new, args.min_seconds))
            a, b = statistics.median(t_old), statistics.median(t_new)
            result["points"].append({"preset": name, "op": "rotate_sum", "k": k, "rotate_hoisted_cc_add": round(a, 1),
                                     "rotate_sum": round(b, 1), "ratio": round(a / b, 3)})
            print(json.dumps(result["points"][-1]), file=sys.stderr, flush=True)
        del eng, keys, ct
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
