"""lt_matmul_bsgs against what it replaces, on one GPU:
    python tools/lt_matmul_bsgs.py [--presets silver,gold] [--shapes 1x4,2x2,4x4] [--diagonals 16,64] [--min-seconds 0.5] [--rounds 5]
                                   [--step-timeout 900] [--flat-key-bytes 8e9]
For every (preset, k_in x k_out, diagonals per block) at level 0, a dense matrix of blocks over the steps 0 .. diagonals - 1 with n1
of encdec.bsgs_split's own choice:
    bsgs     lt_matmul_bsgs(W, cts, keys)                                  one native call, giant groups of up to 4 outputs
    group1   the same with lt_matmul_bsgs_group = 1                        the single giant kernel for every keyed sum
    loop     per output cc_add over linear_transform(cts[i], W[o][i])      k_out k_in BSGS transforms + the additions
    flat     lt_matmul on the same words tagged flat                       one key per step: only where the keys fit --flat-key-bytes
The forms are timed alternately in ONE process per preset (a child of this one, under its own time limit; a preset that fails or
runs out of time ends the run: nothing more is started on the GPU) with device events after a warm-up of each, every timing over at
least --min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over
its rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the key counts, and
the ratios loop / bsgs and group1 / bsgs.
    python tools/lt_matmul_bsgs.py --trace gold:4x4:64 [--calls 10] [--form bsgs|group1|loop|flat] [--out DIR]
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
    """One preset in this process: every shape and block size, the forms alternated; or (--form given by --trace) one form alone."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("lt_matmul_bsgs: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, encdec, presets
    from liberate_fhe_amd.utils import synth
    from tools.hoisted_rotations import timed
    name = args.child
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None
    pool = [synth.ciphertext(eng, 50 + i, 0) for i in range(3)]
    keys = {}

    def keys_for(steps):
        for s in steps:
            if s and s not in keys:
                keys[s] = synth.key_switch_key(eng, 40 + s, origin=f"rotation key:{s}")
        return keys

    key_bytes = sum(t.numel() * 8 for part in keys_for([1])[1].data for comp in part.data for t in comp)
    points = []
    for ndiag in (int(v) for v in args.diagonals.split(",")):
        steps = tuple(range(ndiag))
        n1, babies, giants = encdec.bsgs_split(steps, eng.num_slots)
        with_flat = (ndiag - 1) * key_bytes <= args.flat_key_bytes and (not args.traced or args.form == "flat")
        if args.traced and args.form == "flat" and not with_flat:
            sys.exit(f"lt_matmul_bsgs: {ndiag - 1} flat keys of {key_bytes} bytes do not fit --flat-key-bytes")
        keys_for(steps if with_flat else babies + giants)
        D = [synth.diagonals(eng, 7 + j, 0, steps) for j in range(3)] if with_flat else None
        for shape in args.shapes.split(","):
            k_in, k_out = (int(v) for v in shape.split("x"))
            cts = [pool[i % 3] for i in range(k_in)]
            W = synth.diagonal_matrix_bsgs(eng, 7, 0, steps, n1, k_in, k_out)

            def bsgs(group):
                def run():
                    eng.lt_matmul_bsgs_group = group
                    return eng.lt_matmul_bsgs(W, cts, keys)
                return run

            def loop():
                outs = []
                for row in W:
                    acc = eng.linear_transform(cts[0], row[0], keys)
                    for ct, blk in zip(cts[1:], row[1:]):
                        acc = eng.cc_add(acc, eng.linear_transform(ct, blk, keys))
                    outs.append(acc)
                return outs

            forms = {"bsgs": bsgs(4), "group1": bsgs(1), "loop": loop}
            if with_flat:
                Wf = synth.diagonal_matrix(D, k_in, k_out)
                forms["flat"] = lambda: eng.lt_matmul(Wf, cts, keys)
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
            point = {"preset": name, "k_in": k_in, "k_out": k_out, "diagonals": ndiag, "n1": n1,
                     "keys_bsgs": sum(1 for s in babies + giants if s), "keys_flat": ndiag - 1, **{f: round(med[f], 1) for f in forms},
                     **{f"spread_{f}": round(spread[f], 4) for f in forms}, "loop_over_bsgs": round(med["loop"] / med["bsgs"], 3),
                     "group1_over_bsgs": round(med["group1"] / med["bsgs"], 3)}
            points.append(point)
            print(json.dumps(point), file=sys.stderr, flush=True)
        del D
        if with_flat:      # the flat keys of this block size go before the next one is built
            for s in [s for s in keys if s not in babies + giants]:
                del keys[s]
            torch.cuda.empty_cache()
    print(json.dumps(points))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--shapes", default="1x4,2x2,4x4", help="k_in x k_out, comma-separated")
    ap.add_argument("--diagonals", default="16,64", help="diagonals per block (steps 0 .. diagonals - 1), comma-separated")
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds a child process (one preset, or the trace) may take")
    ap.add_argument("--flat-key-bytes", type=float, default=8e9, help="the flat form is timed where its keys fit this many bytes")
    ap.add_argument("--trace", default=None, help="preset:k_inxk_out:diagonals — one form alone, --calls times, in a fresh child under rocprofv3")
    ap.add_argument("--form", default="bsgs", choices=("bsgs", "group1", "loop", "flat"))
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "lt_matmul_bsgs_trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)       # the preset this process measures
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    me = [sys.executable, os.path.abspath(__file__), "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds),
          "--flat-key-bytes", str(args.flat_key_bytes)]
    if args.trace:
        name, shape, ndiag = args.trace.split(":")
        os.makedirs(args.out, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.out, "--"] + me + ["--child", name, "--shapes", shape, "--diagonals", ndiag,
                                                                                    "--traced", "--form", args.form, "--calls", str(args.calls)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"lt_matmul_bsgs: the trace of {args.trace} ran out of its {args.step_timeout} s; nothing more is started")
        sys.exit(r.returncode)
    result = {"unit": "us per k_in x k_out matrix of blocks of `diagonals` diagonals (steps 0 .. diagonals - 1), level 0", "points": []}
    for name in args.presets.split(","):
        try:
            r = subprocess.run(me + ["--child", name, "--shapes", args.shapes, "--diagonals", args.diagonals], cwd=ROOT,
                               stdout=subprocess.PIPE, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            sys.exit(f"lt_matmul_bsgs: preset {name} ran out of its {args.step_timeout} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"lt_matmul_bsgs: preset {name} ended with status {r.returncode}; nothing more is started")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
