"""pc_matmul_batch against the loop of pc_matmul calls it replaces, on one GPU:
    python tools/pc_matmul_batch.py [--presets silver,gold] [--shapes 8x8,16x16,32x32] [--tokens 2,4,8] [--ab] [--min-seconds 0.3]
                                    [--rounds 5] [--step-timeout 900]
For every (preset, k_in x k_out, B) at level 0, a dense layer applied to B token vectors of k_in ciphertexts each:
    batch    pc_matmul_batch(W, X)                   groups of pc_matmul_batch_sizes (pairs): every plaintext word read once per pair
    loop     [pc_matmul(W, x) for x in X]            B native calls: the whole matrix streamed B times
and with --ab, at the token counts that are multiples of 4, groups of FOUR tokens (pc_matmul_batch_sizes = (4, 2)) covered as
    batch_4tok   tiles of 2 tokens, one native call per four: pc_matmulb_kernel<GO, 2> twice    (the entry's default)
    batch_4x4    ONE launch of pc_matmulb_kernel<GO, 4> per group of outputs                     (lf_tune(LF_TUNE_PC_MATMUL_TILE, 1))
    batch_2x4    .. with 4 outputs as two launches of pc_matmulb_kernel<2, 4>                    (lf_tune(LF_TUNE_PC_MATMUL_TILE, 2))
EVERY weight of the layer is its OWN encode_plain object, k_out * k_in of them, and every ciphertext of every token its own
tensor: tools/pc_matmul.py builds its layers from three plaintexts repeated, 55 MB at gold, which stay in the last-level cache,
so its timings say little about the plaintext stream of a layer whose weights are all different — and that stream is what a
group of tokens shares.  A shape whose operands do not fit the device is reported and dropped, never shrunk.
Each preset is measured in a child process of its own under a time limit (--step-timeout); a child that fails or runs out of
time ends the run: nothing more is started on the GPU.  Inside a child the forms of a point are timed alternately with device
events after a warm-up of each, every timing over at least --min-seconds of work, --rounds rounds; the median is kept and
every form's own run-to-run spread ((max - min) / median over its rounds) is reported beside it.  Prints one JSON line:
microseconds per layer call over all B tokens for each form, the spreads, and the ratio loop / form.
    python tools/pc_matmul_batch.py --trace gold:16x16:4 [--calls 10] [--form batch|loop] [--out DIR]
starts a FRESH child process that runs only that form at that point, under rocprofv3's kernel trace (--kernel-trace --stats,
the program behind `--`), under the same time limit, and prints the kernels' launches and microseconds per call.
Synthetic ciphertexts (utils/synth.py, rolled on the device into tensors of their own) and random messages: the kernels do not
look at the values."""
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

LF_TUNE_PC_MATMUL_TILE = 6


def child(args):
    """One preset in this process: every shape and token count, the forms alternated; or (--form given by --trace) one form alone."""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("pc_matmul_batch: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd._native import lib
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    from tools.hoisted_rotations import timed
    name = args.child
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and eng._native_level(1) is not None
    rng = np.random.default_rng(3)
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    Bs = [int(v) for v in args.tokens.split(",")]
    rows = len(eng.ntt.p.destination_arrays[0][0])
    poly = rows * eng.ctx.N * 8
    free = torch.cuda.mem_get_info()[0]

    def fits(k_in, k_out, B):
        # weights + tokens + outputs of both forms alive at once + the workspace of a group of 4
        need = (k_in * k_out + 2 * B * k_in + 2 * 2 * B * k_out + 4 * (2 * min(k_in, 16) + 2 * k_out)) * poly
        return need < 0.8 * free

    kept = [(s, B) for s in shapes for B in Bs if fits(*s, B)]
    for s in shapes:
        for B in Bs:
            if (s, B) not in kept:
                print(json.dumps({"preset": name, "k_in": s[0], "k_out": s[1], "B": B, "dropped": "operands do not fit the device"}),
                      file=sys.stderr, flush=True)
    if not kept:
        print(json.dumps([]))
        return
    kin_max, kout_max = max(s[0] for s, _ in kept), max(s[1] for s, _ in kept)
    B_max = max(B for _, B in kept)
    t0 = time.time()
    Wall = [[eng.encode_plain(rng.uniform(-1, 1, eng.num_slots), 0) for _ in range(kin_max)] for _ in range(kout_max)]
    base = [synth.ciphertext(eng, 50 + i, 0) for i in range(3)]

    def own(ct, shift):
        return ct._replace(data=tuple([torch.roll(comp[0], shift, 1).contiguous()] for comp in ct.data))

    Xall = [[own(base[(t + i) % 3], 1 + t * kin_max + i) for i in range(kin_max)] for t in range(B_max)]
    torch.cuda.synchronize()
    print(f"{name}: {kout_max * kin_max} plaintexts and {B_max * kin_max} ciphertexts in {time.time() - t0:.1f} s", file=sys.stderr, flush=True)
    assert len({pt.data[0].data_ptr() for row in Wall for pt in row}) == kout_max * kin_max

    def tuned(tile, sizes, fn):
        def f():
            old_sizes, eng.pc_matmul_batch_sizes = eng.pc_matmul_batch_sizes, sizes
            lib.lf_tune(LF_TUNE_PC_MATMUL_TILE, tile)
            try:
                return fn()
            finally:
                lib.lf_tune(LF_TUNE_PC_MATMUL_TILE, 0)
                eng.pc_matmul_batch_sizes = old_sizes
        return f

    points = []
    for (k_in, k_out), B in kept:
        W = [row[:k_in] for row in Wall[:k_out]]
        X = [tok[:k_in] for tok in Xall[:B]]
        batch = lambda: eng.pc_matmul_batch(W, X)
        forms = {"batch": batch, "loop": lambda: [eng.pc_matmul(W, x) for x in X]}
        if args.ab and B % 4 == 0 and not args.traced:
            forms.update({"batch_4tok": tuned(0, (4, 2), batch), "batch_4x4": tuned(1, (4, 2), batch), "batch_2x4": tuned(2, (4, 2), batch)})
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
        point = {"preset": name, "k_in": k_in, "k_out": k_out, "B": B, **{f: round(med[f], 1) for f in forms},
                 **{f"spread_{f}": round(spread[f], 4) for f in forms},
                 **{f"loop_over_{f}": round(med["loop"] / med[f], 3) for f in forms if f != "loop"}}
        points.append(point)
        print(json.dumps(point), file=sys.stderr, flush=True)
    print(json.dumps(points))


def summarize(args):
    """The kernels of the traced child, largest first: launches and microseconds per call of the form.  The child's set-up (the
    encode_plain of every weight, the copies of the ciphertexts) is in the trace too: its kernels show up with launch counts that
    are no multiple of --calls or under names the op does not launch."""
    import csv
    import glob
    rows = []
    for path in glob.glob(os.path.join(args.out, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    if not rows:      # (a rocprofv3 that writes its database whatever format is asked for)
        import sqlite3
        for path in glob.glob(os.path.join(args.out, "**", "*_results.db"), recursive=True):
            q = "select name, count(*), sum(end - start) from kernels group by name"
            rows += [{"Name": n, "Calls": c, "TotalDurationNs": t} for n, c, t in sqlite3.connect(path).execute(q)]
    if not rows:
        sys.exit(f"pc_matmul_batch: no kernel statistics under {args.out}")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    result = {"point": args.trace, "form": args.form, "calls": args.calls, "unit": "us per call", "kernel_us_per_call": round(total / 1000 / args.calls, 1),
              "kernels": []}
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:16]:
        result["kernels"].append({"kernel": r["Name"][:110], "launches_per_call": int(r["Calls"]) / args.calls,
                                  "us": round(float(r["TotalDurationNs"]) / 1000 / args.calls, 1),
                                  "share": round(float(r["TotalDurationNs"]) / total, 4)})
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--shapes", default="8x8,16x16,32x32", help="k_in x k_out, comma-separated")
    ap.add_argument("--tokens", default="2,4,8", help="token vectors per call (B), comma-separated")
    ap.add_argument("--ab", action="store_true", help="also time groups of four tokens under every tile")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child process (one preset, or the trace) may take")
    ap.add_argument("--trace", default=None, help="preset:k_inxk_out:B — one form alone, --calls times, in a fresh child under rocprofv3")
    ap.add_argument("--form", default="batch", choices=("batch", "loop"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "pc_matmul_batch_trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)       # the preset this process measures
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    me = [sys.executable, os.path.abspath(__file__), "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds)]
    if args.trace:
        name, shape, B = args.trace.split(":")
        os.makedirs(args.out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", args.out, "--"] + me + [
            "--child", name, "--shapes", shape, "--tokens", B, "--traced", "--form", args.form, "--calls", str(args.calls)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"pc_matmul_batch: the trace ran out of its {args.step_timeout} s")
        if r.returncode != 0:
            sys.exit(f"pc_matmul_batch: the traced run ended with status {r.returncode}")
        return summarize(args)
    result = {"unit": "us per layer of k_in x k_out plaintext-ciphertext products over B token vectors, level 0", "points": []}
    for name in args.presets.split(","):
        try:
            r = subprocess.run(me + ["--child", name, "--shapes", args.shapes, "--tokens", args.tokens] + (["--ab"] if args.ab else []),
                               cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"pc_matmul_batch: preset {name} ran out of its {args.step_timeout} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"pc_matmul_batch: preset {name} ended with status {r.returncode}; nothing more is started")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
