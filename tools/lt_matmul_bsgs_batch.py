"""lt_matmul_bsgs_batch against the loop of lt_matmul_bsgs it replaces, on one GPU:
    python tools/lt_matmul_bsgs_batch.py [--presets silver,gold] [--shapes 4x4x64x8,2x2x16x4,1x4x64x8] [--tokens 2,4,8] [--ab]
                                         [--min-seconds 0.3] [--rounds 5] [--step-seconds 420]
    python tools/lt_matmul_bsgs_batch.py --trace gold:4x4x64x8:4 [--form batch|loop] [--calls 5] [--out DIR]
For every preset at level 0, every shape k_out x k_in x d x n1 (a k_out x k_in matrix of blocks of d diagonals, steps 0 .. d - 1
over baby steps of n1: n1 - 1 baby keys and d / n1 - 1 giant keys) and every B of --tokens, B token vectors of k_in ciphertexts:
    batch    lt_matmul_bsgs_batch(W, X, keys)            groups of the engine's lt_matmul_bsgs_batch_sizes: every baby key read once
                                                         per group, every diagonal once per tile of two tokens, every giant key
                                                         once per chunk of 4 (token, output) members
    loop     [lt_matmul_bsgs(W, x, keys) for x in X]     B native calls: every key and every diagonal streamed B times
and with --ab one more form per group size the backend takes (batch_4, batch_2: the engine's sizes set to that size alone).
Every block of the matrix is its OWN diagonals object with its own pack in device memory (the words of one synthetic block, copied
on the device: 1024 gold diagonals are 19 GB, too many to draw on the host) and every ciphertext its own tensor, so the diagonal
stream a group shares is as long as that of a layer whose weights are all different.
Each preset is measured in a child process of its own under `timeout -k 10` (--step-seconds); a child that fails ends the run.
Inside a child the forms of a point are timed alternately with device events after a warm-up of each, every timing over at least
--min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its
rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratio loop / form and
whether the form wins by more than the two spreads combined.  Synthetic keys, diagonals and ciphertexts (utils/synth.py): the
kernels do not look at the values.
--trace preset:shape:B runs ONE form of one point alone, --calls times, in a fresh child under `rocprofv3 --kernel-trace --stats`
(tables under --out): the split of a call over its kernels."""
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
        sys.exit("lt_matmul_bsgs_batch: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    from tools.lt_matmul_batch import measure
    name = args.child
    shapes = [tuple(int(v) for v in s.lower().split("x")) for s in args.shapes.split(",")]
    tokens = sorted({int(b) for b in args.tokens.split(",")})
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and hasattr(eng.backend, "lt_matmul_bsgs_batch_call")
    imax = max(k_in for _, k_in, _, _ in shapes)
    steps = sorted({s for _, _, d, n1 in shapes for s in list(range(1, n1)) + list(range(n1, d, n1))})
    keys = [synth.key_switch_key(eng, 100 + s, origin=f"rotation key:{s}") for s in steps]
    pool = [[synth.ciphertext(eng, 7 + imax * t + i, 0) for i in range(imax)] for t in range(max(tokens))]
    shipped = tuple(type(eng).lt_matmul_bsgs_batch_sizes)

    def sized(sizes, fn):
        def run():
            eng.lt_matmul_bsgs_batch_sizes = sizes
            try:
                return fn()
            finally:
                eng.lt_matmul_bsgs_batch_sizes = shipped
        return run

    def own_copy(block):
        """a diagonals object of its own: the same tags, its own pack"""
        packs = [pk.clone() for pk in eng._diag_pack(block)]
        out = block._replace(data=[[pk[j] for pk in packs] for j in range(len(block.data))])
        eng._remember_diag_pack(out, packs, own=True)
        return out

    points = []
    for k_out, k_in, d, n1 in shapes:
        first = synth.diagonals_bsgs(eng, 3, 0, range(d), n1)
        W = [[first if o == i == 0 else own_copy(first) for i in range(k_in)] for o in range(k_out)]
        assert len({eng._diag_pack(b)[0].data_ptr() for row in W for b in row}) == k_out * k_in
        for B in tokens:
            X = [tok[:k_in] for tok in pool[:B]]
            batch = lambda: eng.lt_matmul_bsgs_batch(W, X, keys)
            forms = {"batch": batch, "loop": lambda: [eng.lt_matmul_bsgs(W, x, keys) for x in X]}
            if args.traced:
                for _ in range(args.calls):
                    forms[args.form]()
                torch.cuda.synchronize()
                continue
            if args.ab:
                forms.update({f"batch_{s}": sized((s,), batch) for s in eng.backend.lt_matmul_bsgs_batch_sizes if s <= B})
            want = forms["loop"]()                       # (the timed forms give the same words)
            for f, fn in forms.items():
                got = fn()
                assert all(torch.equal(x.data[c][0], y.data[c][0]) for a, b in zip(got, want) for x, y in zip(a, b) for c in range(2)), f
                del got
            del want
            points.append({"preset": name, "shape": f"{k_out}x{k_in}x{d}", "n1": n1, "tokens": B, "sizes": list(shipped),
                           **measure(forms, args.min_seconds, args.rounds)})
            print(json.dumps(points[-1]), file=sys.stderr, flush=True)
        del W
        torch.cuda.empty_cache()
    print(json.dumps(points))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--shapes", default="4x4x64x8,2x2x16x4,1x4x64x8", help="k_out x k_in x diagonals per block x n1, comma-separated")
    ap.add_argument("--tokens", default="2,4,8", help="token vectors per call (B), comma-separated")
    ap.add_argument("--ab", action="store_true", help="also time every group size the backend takes on its own")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=420, help="time limit of each child process")
    ap.add_argument("--trace", default=None, help="preset:shape:B — one form alone, --calls times, in a fresh child under rocprofv3")
    ap.add_argument("--form", default="batch", choices=("batch", "loop"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "lt_matmul_bsgs_batch_trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.trace:
        name, shape, B = args.trace.split(":")
        os.makedirs(args.out, exist_ok=True)
        cmd = ["timeout", "-k", "10", str(args.step_seconds), "rocprofv3", "--kernel-trace", "--stats", "-d", args.out, "--", sys.executable,
               os.path.abspath(__file__), "--child", name, "--shapes", shape, "--tokens", B, "--traced", "--form", args.form, "--calls",
               str(args.calls)]
        sys.exit(subprocess.run(cmd, cwd=ROOT).returncode)
    result = {"unit": "us per call (level 0)", "points": []}
    for name in args.presets.split(","):
        cmd = ["timeout", "-k", "10", str(args.step_seconds), sys.executable, os.path.abspath(__file__), "--child", name, "--shapes",
               args.shapes, "--tokens", args.tokens, "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds)]
        r = subprocess.run(cmd + (["--ab"] if args.ab else []), cwd=ROOT, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:      # (a time limit, a fault or an abort: nothing more is started on the GPU)
            print(json.dumps(result))
            sys.exit(f"lt_matmul_bsgs_batch: the run of {name} ended with status {r.returncode}")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
