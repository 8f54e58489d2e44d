"""Hoisted rotations against a loop of rotate_single (one ciphertext, k steps), in one process:
    python tools/hoisted_rotations.py [--presets silver,gold] [--ks 1,2,4,8,16] [--min-seconds 0.5]
For every (preset, k) the two forms are timed alternately with device events after a warm-up, each over at least
--min-seconds of work, three rounds, the median kept.  Prints one JSON line: microseconds per rotation for each form and
their ratio (loop / hoisted).  Synthetic keys and ciphertexts (utils/synth.py): the kernels do not look at the values."""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
warnings.filterwarnings("ignore")


def timed(fn, min_seconds):
    import torch
    fn()
    torch.cuda.synchronize()
    reps, ms = 1, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 1000 * min_seconds:
            return ms * 1000 / reps
        reps = max(reps + 1, int(reps * 1.2 * 1000 * min_seconds / max(ms, 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("hoisted_rotations: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    ks = [int(k) for k in args.ks.split(",")]
    result = {"unit": "us per rotation", "points": []}
    for name in args.presets.split(","):
        params = {k: v for k, v in presets.params[name].items() if k != "devices"}
        eng = ckks_engine(devices=["cuda:0"], **params)
        keys = [synth.key_switch_key(eng, 100 + i, origin=f"rotation key:{i + 1}") for i in range(max(ks))]
        ct = synth.ciphertext(eng, 7, 0)
        for k in ks:
            loop = lambda: [eng.rotate_single(ct, key) for key in keys[:k]]
            hoist = lambda: eng.rotate_hoisted(ct, keys[:k])
            loop(), hoist()
            t_loop, t_hoist = [], []
            for _ in range(args.rounds):
                t_loop.append(timed(loop, args.min_seconds) / k)
                t_hoist.append(timed(hoist, args.min_seconds) / k)
            a, b = statistics.median(t_loop), statistics.median(t_hoist)
            result["points"].append({"preset": name, "k": k, "rotate_single_loop": round(a, 1), "rotate_hoisted": round(b, 1),
                                     "ratio": round(a / b, 3)})
            print(json.dumps(result["points"][-1]), file=sys.stderr, flush=True)
        del eng, keys, ct
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
