"""lt_matmul_batch against the loop of lt_matmul it replaces, on one GPU:
    python tools/lt_matmul_batch.py [--presets silver,gold] [--shapes 4x4x8,2x2x16] [--tokens 2,4,8] [--ab] [--min-seconds 0.3]
                                    [--rounds 5] [--step-seconds 420]
For every preset at level 0, every shape k_out x k_in x d (a k_out x k_in matrix of blocks of d diagonals: steps 0 .. d - 1, so
d - 1 rotation keys per column) and every B of --tokens, B token vectors of k_in ciphertexts each:
    batch    lt_matmul_batch(W, X, keys)              groups of the engine's lt_matmul_batch_sizes: every key and diagonal read once
                                                      per group resp. per tile of two tokens
    loop     [lt_matmul(W, x, keys) for x in X]       B native calls: every key and every diagonal streamed B times
and with --ab one more form per group size the backend takes (batch_4, batch_2: the engine's sizes set to that size alone).
Every block of the matrix is its OWN diagonals object and every ciphertext its own tensor, so the diagonal stream a group shares
is as long as that of a layer whose weights are all different.
Each preset is measured in a child process of its own under `timeout -k 10` (--step-seconds); a child that fails ends the run.
Inside a child the forms of a point are timed alternately with device events after a warm-up of each, every timing over at least
--min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its
rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratio loop / form and
whether the form wins by more than the two spreads combined.  Synthetic keys, diagonals and ciphertexts (utils/synth.py): the
kernels do not look at the values."""
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


def measure(forms, min_seconds, rounds):
    from tools.hoisted_rotations import timed
    for fn in forms.values():
        fn()
    times = {f: [] for f in forms}
    for _ in range(rounds):
        for f, fn in forms.items():
            times[f].append(timed(fn, min_seconds))
    med = {f: statistics.median(t) for f, t in times.items()}
    out = {f: round(med[f], 1) for f in forms}
    spread = {f: (max(t) - min(t)) / med[f] for f, t in times.items()}
    out.update({f"spread_{f}": round(s, 4) for f, s in spread.items()})
    for f in forms:
        if f != "loop":
            out[f"loop_over_{f}"] = round(med["loop"] / med[f], 3)
            out[f"{f}_wins"] = bool(med["loop"] / med[f] > 1 + spread["loop"] + spread[f])
    return out


def child(args):
    """one preset in this process"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("lt_matmul_batch: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    name = args.child
    shapes = [tuple(int(v) for v in s.lower().split("x")) for s in args.shapes.split(",")]
    tokens = sorted({int(b) for b in args.tokens.split(",")})
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and hasattr(eng.backend, "lt_matmul_batch_native")
    dmax, imax = max(d for _, _, d in shapes), max(k_in for _, k_in, _ in shapes)
    keys = [synth.key_switch_key(eng, 100 + s, origin=f"rotation key:{s}") for s in range(1, dmax)]
    pool = [[synth.ciphertext(eng, 7 + imax * t + i, 0) for i in range(imax)] for t in range(max(tokens))]
    shipped = tuple(type(eng).lt_matmul_batch_sizes)

    def sized(sizes, fn):
        def run():
            eng.lt_matmul_batch_sizes = sizes
            try:
                return fn()
            finally:
                eng.lt_matmul_batch_sizes = shipped
        return run

    points = []
    for k_out, k_in, d in shapes:
        W = [[synth.diagonals(eng, 3 + o * k_in + i, 0, range(d)) for i in range(k_in)] for o in range(k_out)]
        for B in tokens:
            X = [tok[:k_in] for tok in pool[:B]]
            batch = lambda: eng.lt_matmul_batch(W, X, keys)
            forms = {"batch": batch, "loop": lambda: [eng.lt_matmul(W, x, keys) for x in X]}
            if args.ab:
                forms.update({f"batch_{s}": sized((s,), batch) for s in eng.backend.lt_matmul_batch_sizes if s <= B})
            want = forms["loop"]()                       # (the timed forms give the same words)
            for f, fn in forms.items():
                got = fn()
                assert all(torch.equal(x.data[c][0], y.data[c][0]) for a, b in zip(got, want) for x, y in zip(a, b) for c in range(2)), f
                del got
            del want
            points.append({"preset": name, "shape": f"{k_out}x{k_in}x{d}", "tokens": B, "sizes": list(shipped),
                           **measure(forms, args.min_seconds, args.rounds)})
            print(json.dumps(points[-1]), file=sys.stderr, flush=True)
        del W
        torch.cuda.empty_cache()
    print(json.dumps(points))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--shapes", default="4x4x8,2x2x16", help="k_out x k_in x diagonals per block, comma-separated")
    ap.add_argument("--tokens", default="2,4,8", help="token vectors per call (B), comma-separated")
    ap.add_argument("--ab", action="store_true", help="also time every group size the backend takes on its own")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=420, help="time limit of each child process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"unit": "us per call (level 0)", "points": []}
    for name in args.presets.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--child", name, "--shapes",
               args.shapes, "--tokens", args.tokens, "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd + (["--ab"] if args.ab else []), cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:      # (a time limit, a fault or an abort: nothing more is started on the GPU)
            print(json.dumps(result))
            sys.exit(f"lt_matmul_batch: the run of {name} ended with status {r.returncode}")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
