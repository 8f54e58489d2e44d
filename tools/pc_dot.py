"""pc_dot against the two ways to write a sum of plaintext-ciphertext products without it, on one GPU:
    python tools/pc_dot.py [--presets silver,gold] [--ks 1,2,4,8,16] [--min-seconds 0.5] [--rounds 5] [--step-timeout 600]
For every (preset, k) at level 0, k terms over three plaintexts / messages and three ciphertexts:
    dot      pc_dot(pairs)                                   plaintexts encoded once, one rescale for the sum
    mc       k x mc_mult(m, ct), then the cc_add chain       the reference-shaped loop: encodes on every call
    pc       k x pc_mult(pt, ct), then the cc_add chain      plaintexts encoded once, a rescale per term
The three forms are timed alternately in ONE process per preset (a child of this one, under its own time limit; a preset that
fails or runs out of time ends the run: nothing more is started on the GPU) with device events after a warm-up of each, every
timing over at least --min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread
((max - min) / median over its rounds) is reported beside it.  Prints one JSON line: microseconds per sum for each form, the
spreads, and the ratios mc / dot and pc / dot.
    python tools/pc_dot.py --trace gold:8 [--calls 10] [--form dot|mc|pc] [--out DIR]
starts a FRESH child process that runs only that form at that point, under rocprofv3's kernel trace (--kernel-trace --stats,
the program behind `--`), under the same time limit.
Synthetic ciphertexts (utils/synth.py) and random messages: the kernels do not look at the values."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")

SLOTS = ((0, 0), (1, 1), (0, 2), (2, 0), (1, 0), (2, 2), (0, 1), (1, 2), (2, 1))


def child(args):
    """One preset in this process: every k, the forms alternated; or (--form given by --trace) one form alone."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("pc_dot: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    from tools.hoisted_rotations import timed
    name = args.child
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and eng._native_level(1) is not None
    rng = np.random.default_rng(3)
    ms = [rng.uniform(-1, 1, eng.num_slots) for _ in range(3)]
    pts = [eng.encode_plain(m, 0) for m in ms]
    cts = [synth.ciphertext(eng, 50 + i, 0) for i in range(3)]
    points = []
    for k in [int(k) for k in args.ks.split(",")]:
        slots = (SLOTS * (k // len(SLOTS) + 1))[:k]

        def chain(products):
            acc = products[0]
            for p in products[1:]:
                acc = eng.cc_add(acc, p)
            return acc

        forms = {"dot": lambda: eng.pc_dot([(pts[i], cts[j]) for i, j in slots]),
                 "mc": lambda: chain([eng.mc_mult(ms[i], cts[j]) for i, j in slots]),
                 "pc": lambda: chain([eng.pc_mult(pts[i], cts[j]) for i, j in slots])}
        if args.traced:
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
                 "mc_over_dot": round(med["mc"] / med["dot"], 3), "pc_over_dot": round(med["pc"] / med["dot"], 3)}
        points.append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(points))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds a child process (one preset, or the trace) may take")
    ap.add_argument("--trace", default=None, help="preset:k — one form alone, --calls times, in a fresh child under rocprofv3")
    ap.add_argument("--form", default="dot", choices=("dot", "mc", "pc"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "pc_dot_trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)       # the preset this process measures
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    me = [sys.executable, os.path.abspath(__file__), "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds)]
    if args.trace:
        name, k = args.trace.split(":")
        os.makedirs(args.out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.out, "--"] + me + ["--child", name, "--ks", k, "--traced", "--form", args.form,
                                                                                    "--calls", str(args.calls)]
        r = subprocess.run(cmd, cwd=ROOT, timeout=args.step_timeout)
        sys.exit(r.returncode)
    result = {"unit": "us per sum of k plaintext-ciphertext products, level 0", "points": []}
    for name in args.presets.split(","):
        try:
            r = subprocess.run(me + ["--child", name, "--ks", args.ks], cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"pc_dot: preset {name} ran out of its {args.step_timeout} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"pc_dot: preset {name} ended with status {r.returncode}; nothing more is started")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
