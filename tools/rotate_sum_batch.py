"""rotate_sum_batch / inner_sum_batch against the loops of rotate_sum / inner_sum they replace, on one GPU:
    python tools/rotate_sum_batch.py [--presets silver,gold] [--cts 2,4,8,16] [--ks 3,7] [--n 64] [--radix 4] [--min-seconds 0.3] [--rounds 5]
For every preset at level 0 and every (B, k) of --cts x --ks, B ciphertexts under k rotation keys + the self term:
    batch    rotate_sum_batch(cts, keys)                  groups of rsum_batch_sizes: every key read once per group
    loop     [rotate_sum(ct, keys) for ct in cts]
and for every B of --cts the same pair for inner_sum_batch(cts, n, keys, radix=radix) | [inner_sum(ct, n, keys, radix=radix)].
Each preset is measured in a child process of its own under `timeout -k 10` (--step-seconds); a child that fails ends the run.
Inside a child the two forms of a point are timed alternately with device events after a warm-up of each, every timing over at
least --min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median
over its rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratio
loop / batch and whether the batch wins by more than the two spreads combined.  Synthetic keys and ciphertexts (utils/synth.py):
the kernels do not look at the values."""
import argparse
import json
import os
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")


def child(args):
    """one preset in this process"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("rotate_sum_batch: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    from tools.linear_transform_batch import measure
    name = args.child
    shapes = [(int(b), int(k)) for b in args.cts.split(",") for k in args.ks.split(",")]
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and hasattr(eng.backend, "rotate_sum_batch_native")
    kmax, bmax = max(k for _, k in shapes), max(b for b, _ in shapes)
    keys = [synth.key_switch_key(eng, 100 + i, origin=f"rotation key:{i + 1}") for i in range(kmax)]
    cts = [synth.ciphertext(eng, 7 + i, 0) for i in range(bmax)]
    same = lambda a, b: all(torch.equal(x.data[c][0], y.data[c][0]) for x, y in zip(a, b) for c in range(2))
    points = []

    def point(tag, forms):
        assert same(forms["batch"](), forms["loop"]())      # (the timed forms give the same words)
        points.append({"preset": name, **tag, **measure(forms, args.min_seconds, args.rounds)})
        print(json.dumps(points[-1]), file=sys.stderr, flush=True)

    for B, k in sorted(shapes, key=lambda s: (s[1], s[0])):
        point({"op": "rotate_sum", "cts": B, "k": k},
              {"batch": lambda: eng.rotate_sum_batch(cts[:B], keys[:k]), "loop": lambda: [eng.rotate_sum(ct, keys[:k]) for ct in cts[:B]]})
    del keys
    if args.n > 1:
        steps = eng.inner_sum_steps(args.n, 1, args.radix)
        ikeys = {s: synth.key_switch_key(eng, 200 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}
        for B in sorted({b for b, _ in shapes}):
            point({"op": "inner_sum", "cts": B, "n": args.n, "radix": args.radix},
                  {"batch": lambda: eng.inner_sum_batch(cts[:B], args.n, ikeys, radix=args.radix),
                   "loop": lambda: [eng.inner_sum(ct, args.n, ikeys, radix=args.radix) for ct in cts[:B]]})
    print(json.dumps(points))


def run_child(extra, seconds):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), *extra]
    return subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--cts", default="2,4,8,16")
    ap.add_argument("--ks", default="3,7")
    ap.add_argument("--n", type=int, default=64, help="inner_sum_batch's n (0: skip it)")
    ap.add_argument("--radix", type=int, default=4)
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=420, help="time limit of each child process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"unit": "us per call (level 0; rotate_sum: k keys + self; inner_sum: n, radix)", "points": []}
    for name in args.presets.split(","):
        r = run_child(["--child", name, "--cts", args.cts, "--ks", args.ks, "--n", str(args.n), "--radix", str(args.radix),
                       "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds)], args.step_seconds)
        if r.returncode != 0:      # (a time limit, a fault or an abort: nothing more is started on the GPU)
            print(json.dumps(result))
            sys.exit(f"rotate_sum_batch: the run of {name} ended with status {r.returncode}")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
