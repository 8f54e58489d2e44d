"""Compact plaintexts (compact_plain: fp64-class rows as 6-byte planes) against the raw ones in pc_matmul and pc_matmul_batch, on one GPU:
    python tools/compact_plain.py [--presets silver,gold] [--shapes 8x8,16x16,32x32] [--tokens 1,2,4] [--min-seconds 0.3] [--rounds 5]
                                  [--step-timeout 900]
For every (preset, k_in x k_out, B) at level 0, a dense layer over B token vectors of k_in ciphertexts each (B = 1: pc_matmul;
B >= 2: pc_matmul_batch, pairs of tokens per native call):
    raw       the layer's weights as encode_plain returns them                          lf_pc_matmul / lf_pc_matmul_batch
    compact   compact_plain of the same weights                                         lf_pc_matmul_batch_planes
EVERY weight of the layer is its OWN plaintext, k_out * k_in of them in each form (tools/pc_matmul_batch.py says why), and every
ciphertext of every token its own tensor.  A shape whose operands do not fit the device is reported and dropped, never shrunk.
Both presets are measured in ONE child process, one after the other, under a time limit (--step-timeout); a child that fails or runs
out of time ends the run.  The two forms of a point are timed alternately with device events after a warm-up of each, every timing
over at least --min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) /
median over its rounds) is reported beside it.  Prints one JSON line: microseconds per call for both forms, raw / compact, the
spreads, the bytes of the layer's weights both ways, and the packer's microseconds per plaintext (compact_plain of one weight).
Synthetic ciphertexts and random messages: the kernels do not look at the values."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.filterwarnings("ignore")


def measure(name, args):
    import numpy as np
    import torch
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    from tools.hoisted_rotations import timed
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._pc_planes_native(0) is not None
    rng = np.random.default_rng(3)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    Bs = [int(v) for v in args.tokens.split(",")]
    rows = len(eng.ntt.p.destination_arrays[0][0])
    poly = rows * eng.ctx.N * 8
    free = torch.cuda.mem_get_info()[0]

    def fits(k_in, k_out, B):
        # weights in both forms + tokens + outputs of both forms alive at once + the workspace of a pair
        need = (2 * k_in * k_out + 2 * B * k_in + 2 * 2 * B * k_out + 2 * (2 * min(k_in, 16) + 2 * k_out)) * poly
        return need < 0.8 * free

    kept = [(s, B) for s in shapes for B in Bs if fits(*s, B)]
    for s in shapes:
        for B in Bs:
            if (s, B) not in kept:
                print(json.dumps({"preset": name, "k_in": s[0], "k_out": s[1], "B": B, "dropped": "operands do not fit the device"}),
                      file=sys.stderr, flush=True)
    if not kept:
        return []
    kin_max, kout_max = max(s[0] for s, _ in kept), max(s[1] for s, _ in kept)
    B_max = max(B for _, B in kept)
    t0 = time.time()
    Wall = [[eng.encode_plain(rng.uniform(-1, 1, eng.num_slots), 0) for _ in range(kin_max)] for _ in range(kout_max)]
    Kall = [[eng.compact_plain(pt) for pt in row] for row in Wall]
    base = [synth.ciphertext(eng, 50 + i, 0) for i in range(3)]

    def own(ct, shift):
        return ct._replace(data=tuple([torch.roll(comp[0], shift, 1).contiguous()] for comp in ct.data))

    Xall = [[own(base[(t + i) % 3], 1 + t * kin_max + i) for i in range(kin_max)] for t in range(B_max)]
    torch.cuda.synchronize()
    print(f"{name}: {kout_max * kin_max} plaintexts in both forms and {B_max * kin_max} ciphertexts in {time.time() - t0:.1f} s",
          file=sys.stderr, flush=True)
    raw_bytes, compact_bytes = Wall[0][0].data[0].numel() * 8, Kall[0][0].data[0].numel() * 8
    pack = [timed(lambda: eng.compact_plain(Wall[0][0]), args.min_seconds) for _ in range(args.rounds)]
    points = []
    for (k_in, k_out), B in kept:
        X = [tok[:k_in] for tok in Xall[:B]]
        forms = {}
        for form, M in (("raw", Wall), ("compact", Kall)):
            W = [row[:k_in] for row in M[:k_out]]
            forms[form] = (lambda W=W: eng.pc_matmul(W, X[0])) if B == 1 else (lambda W=W: eng.pc_matmul_batch(W, X))
        for fn in forms.values():
            fn()
        times = {f: [] for f in forms}
        for _ in range(args.rounds):
            for f, fn in forms.items():
                times[f].append(timed(fn, args.min_seconds))
        med = {f: statistics.median(t) for f, t in times.items()}
        point = {"preset": name, "k_in": k_in, "k_out": k_out, "B": B, "op": "pc_matmul" if B == 1 else "pc_matmul_batch",
                 **{f: round(med[f], 1) for f in forms},
                 **{f"spread_{f}": round((max(t) - min(t)) / med[f], 4) for f, t in times.items()},
                 "raw_over_compact": round(med["raw"] / med["compact"], 3),
                 "weights_raw_bytes": k_in * k_out * raw_bytes, "weights_compact_bytes": k_in * k_out * compact_bytes,
                 "bytes_ratio": round(compact_bytes / raw_bytes, 4),
                 "pack_us_per_plaintext": round(statistics.median(pack), 1), "spread_pack": round((max(pack) - min(pack)) / statistics.median(pack), 4)}
        points.append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    return points


def child(args):
    """Every preset in this one process, one after the other."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("compact_plain: no GPU")
    import __graft_entry__ as g
    g.build()
    points = []
    for name in args.presets.split(","):
        points += measure(name, args)
    print(json.dumps(points))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--shapes", default="8x8,16x16,32x32", help="k_in x k_out, comma-separated")
    ap.add_argument("--tokens", default="1,2,4", help="token vectors per call (B): 1 is pc_matmul, more pc_matmul_batch")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds the child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    me = [sys.executable, os.path.abspath(__file__), "--child", "--presets", args.presets, "--shapes", args.shapes, "--tokens", args.tokens,
          "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds)]
    try:
        r = subprocess.run(me, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
    except subprocess.TimeoutExpired:
        sys.exit(f"compact_plain: the child ran out of its {args.step_timeout} s")
    if r.returncode != 0:
        sys.exit(f"compact_plain: the child ended with status {r.returncode}")
    print(json.dumps({"unit": "us per call of a k_in x k_out layer over B token vectors, level 0", "points": json.loads(r.stdout.strip().splitlines()[-1])}))


if __name__ == "__main__":
    main()
