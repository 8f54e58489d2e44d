"""lt_matmul against the loop of linear_transform + cc_add it replaces, on one GPU:
    python tools/lt_matmul.py [--presets silver,gold] [--shapes 1x4,2x2,4x4] [--diagonals 8] [--min-seconds 0.5] [--rounds 5] [--step-timeout 600]
For every (preset, k_in x k_out) at level 0, a dense matrix of blocks of --diagonals diagonals each (steps 0 .. diagonals - 1):
    matmul   lt_matmul(W, cts, keys)                                   one native call: the rotations of an input formed once
    loop     per output cc_add over linear_transform(cts[i], W[o][i])  k_out k_in native calls + the additions
The two forms are timed alternately in ONE process per preset (a child of this one, under its own time limit; a preset that
fails or runs out of time ends the run: nothing more is started on the GPU) with device events after a warm-up of each, every
timing over at least --min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread
((max - min) / median over its rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the
spreads, and the ratio loop / matmul.
    python tools/lt_matmul.py --trace gold:4x4 [--calls 10] [--form matmul|loop] [--out DIR]
starts a FRESH child process that runs only that form at that point, under rocprofv3's kernel trace (--kernel-trace --stats,
the program behind `--`), under the same time limit.
Synthetic ciphertexts, keys and diagonals (utils/synth.py): the kernels do not look at the values."""
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


def child(args):
    """One preset in this process: every shape, the forms alternated; or (--form given by --trace) one form alone."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("lt_matmul: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    from tools.hoisted_rotations import timed
    name = args.child
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None
    steps = tuple(range(args.diagonals))
    keys = {s: synth.key_switch_key(eng, 40 + s, origin=f"rotation key:{s}") for s in steps if s}
    D = [synth.diagonals(eng, 7 + j, 0, steps) for j in range(3)]
    pool = [synth.ciphertext(eng, 50 + i, 0) for i in range(3)]
    points = []
    for shape in args.shapes.split(","):
        k_in, k_out = (int(v) for v in shape.split("x"))
        cts = [pool[i % 3] for i in range(k_in)]
        W = synth.diagonal_matrix(D, k_in, k_out)

        def loop():
            outs = []
            for row in W:
                acc = eng.linear_transform(cts[0], row[0], keys)
                for ct, blk in zip(cts[1:], row[1:]):
                    acc = eng.cc_add(acc, eng.linear_transform(ct, blk, keys))
                outs.append(acc)
            return outs

        forms = {"matmul": lambda: eng.lt_matmul(W, cts, keys), "loop": loop}
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
        point = {"preset": name, "k_in": k_in, "k_out": k_out, "diagonals": args.diagonals, **{f: round(med[f], 1) for f in forms},
                 **{f"spread_{f}": round(spread[f], 4) for f in forms}, "loop_over_matmul": round(med["loop"] / med["matmul"], 3)}
        points.append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(points))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--shapes", default="1x4,2x2,4x4", help="k_in x k_out, comma-separated")
    ap.add_argument("--diagonals", type=int, default=8, help="diagonals per block: steps 0 .. diagonals - 1")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds a child process (one preset, or the trace) may take")
    ap.add_argument("--trace", default=None, help="preset:k_inxk_out — one form alone, --calls times, in a fresh child under rocprofv3")
    ap.add_argument("--form", default="matmul", choices=("matmul", "loop"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "lt_matmul_trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)       # the preset this process measures
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    me = [sys.executable, os.path.abspath(__file__), "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds), "--diagonals",
          str(args.diagonals)]
    if args.trace:
        name, shape = args.trace.split(":")
        os.makedirs(args.out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.out, "--"] + me + ["--child", name, "--shapes", shape, "--traced", "--form",
                                                                                    args.form, "--calls", str(args.calls)]
        r = subprocess.run(cmd, cwd=ROOT, timeout=args.step_timeout)
        sys.exit(r.returncode)
    result = {"unit": f"us per k_in x k_out matrix of blocks of {args.diagonals} diagonals, level 0", "points": []}
    for name in args.presets.split(","):
        try:
            r = subprocess.run(me + ["--child", name, "--shapes", args.shapes], cwd=ROOT, stdout=subprocess.PIPE, text=True,
                               timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"lt_matmul: preset {name} ran out of its {args.step_timeout} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"lt_matmul: preset {name} ended with status {r.returncode}; nothing more is started")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
