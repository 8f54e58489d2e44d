"""The flat linear_transform against its baby-step / giant-step form on the same diagonals, in one process:
    python tools/linear_transform_bsgs.py [--presets silver,gold] [--ks 8,16,32,64] [--min-seconds 0.5]
k consecutive steps 0 .. k - 1; the flat form needs k - 1 keys, the BSGS form the keys of the non-zero baby and giant steps of
encdec.bsgs_split's own choice of n1.  For every (preset, k) the two forms are timed alternately with device events after a
warm-up, each over at least --min-seconds of work, three rounds, the median kept.  Prints one JSON line: microseconds per call
for each form, the key counts, n1 and the ratio (flat / BSGS).  The flat keys of the largest k are built once per preset and
freed with it (gold, k = 64: 63 keys of 368 MB).
    python tools/linear_transform_bsgs.py --trace gold:64 [--calls 10] [--form bsgs|flat]
runs only that form at that point (for a kernel trace taken from outside, the program in a process of its own).
Synthetic keys, diagonals and ciphertexts (utils/synth.py): the kernels do not look at the values."""
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
    ap.add_argument("--ks", default="8,16,32,64")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", default=None, help="preset:k — run one form alone, --calls times")
    ap.add_argument("--form", default="bsgs", choices=("bsgs", "flat"))
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("linear_transform_bsgs: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, encdec, presets
    from liberate_fhe_amd.utils import synth
    names, ks = args.presets.split(","), [int(k) for k in args.ks.split(",")]
    if args.trace:
        names, ks = [args.trace.split(":")[0]], [int(args.trace.split(":")[1])]
    result = {"unit": "us per call (k diagonals, steps 0 .. k - 1)", "points": []}
    for name in names:
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        splits = {k: encdec.bsgs_split(range(k), eng.num_slots) for k in ks}
        need = set()
        for k in ks:
            if not (args.trace and args.form == "flat"):
                need |= {s for s in splits[k][1] + splits[k][2] if s}
            if not (args.trace and args.form == "bsgs"):
                need |= set(range(1, k))
        keys = {s: synth.key_switch_key(eng, 100 + s, origin=f"rotation key:{s}") for s in sorted(need)}
        ct = synth.ciphertext(eng, 7, 0)
        for k in ks:
            n1, babies, giants = splits[k]
            flat_d = synth.diagonals(eng, 3, 0, range(k))
            bsgs_d = synth.diagonals_bsgs(eng, 3, 0, range(k), n1)
            flat = lambda: eng.linear_transform(ct, flat_d, keys)
            bsgs = lambda: eng.linear_transform(ct, bsgs_d, keys)
            if args.trace:
                fn = bsgs if args.form == "bsgs" else flat
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                continue
            flat(), bsgs()
            t_flat, t_bsgs = [], []
            for _ in range(args.rounds):
                t_flat.append(timed(flat, args.min_seconds))
                t_bsgs.append(timed(bsgs, args.min_seconds))
            a, b = statistics.median(t_flat), statistics.median(t_bsgs)
            result["points"].append({"preset": name, "k": k, "n1": n1, "keys_flat": k - 1,
                                     "keys_bsgs": sum(1 for s in babies + giants if s), "flat": round(a, 1), "bsgs": round(b, 1),
                                     "ratio": round(a / b, 3)})
            print(json.dumps(result["points"][-1]), file=sys.stderr, flush=True)
            del flat_d, bsgs_d
        del eng, keys, ct
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
