"""linear_transform_batch over baby-step / giant-step diagonals against what a user could do before it, on one GPU:
    python tools/linear_transform_bsgs_batch.py [--presets silver,gold] [--cts 2,4,8,16] [--shapes 64:8,16:4] [--min-seconds 0.3] [--rounds 5]
For every preset at level 0, every shape k:n1 (k diagonals, steps 0 .. k - 1, encoded with bsgs=n1: 64:8 needs 7 + 7 keys) and
every B of --cts, B ciphertexts under the same diagonals:
    batch    linear_transform_batch(cts, diags, keys)     groups of lt_bsgs_batch_sizes: every baby and giant key read once per group
    loop     [linear_transform(ct, diags, keys) for ct in cts]      (what the batch call did before the native entry)
    matmul   lt_matmul_bsgs(W, cts, keys), W the B x B matrix with the block on its diagonal: the giant keys shared across
             the outputs, the baby rotations formed one input at a time
Each preset is measured in a child process of its own under `timeout -k 10` (--step-seconds); a child that fails ends the run.
Inside a child the forms of a point are timed alternately with device events after a warm-up of each, every timing over at least
--min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its
rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratios loop / batch
and matmul / batch, and whether the batch beats the loop by more than the two spreads combined.  --sizes 4 or --sizes 2 measures
the batch with that group size alone (engine.lt_bsgs_batch_sizes), which is how a size is judged on its own.
    python tools/linear_transform_bsgs_batch.py --trace gold:8x64:8 [--calls 10] [--form batch|loop] [--out out/lt_bsgs_batch_trace]
runs one `rocprofv3 --kernel-trace --stats` pass over --calls calls of that point (preset:Bxk:n1) in a process of its own, the
program after `--`, under `timeout -k 10`, and prints the kernels' totals from its statistics, per call and as shares of the
kernel time.  Synthetic keys and ciphertexts (utils/synth.py): the kernels do not look at the values."""
import argparse
import csv
import glob
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
    out["loop_over_batch"] = round(med["loop"] / med["batch"], 3)
    if "matmul" in med:
        out["matmul_over_batch"] = round(med["matmul"] / med["batch"], 3)
    out["batch_wins"] = bool(med["loop"] / med["batch"] > 1 + spread["loop"] + spread["batch"])
    return out


def child(args):
    """one preset (or one point of it, --calls times, for a trace) in this process"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("linear_transform_bsgs_batch: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, encdec, presets
    from liberate_fhe_amd.utils import synth
    name = args.child
    shapes = [tuple(int(v) for v in s.split(":")) for s in args.shapes.split(",")]
    Bs = sorted(int(b) for b in args.cts.split(","))
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and hasattr(eng.backend, "linear_transform_bsgs_batch_native")
    if args.sizes:
        eng.lt_bsgs_batch_sizes = tuple(int(s) for s in args.sizes.split(","))
    cts = [synth.ciphertext(eng, 7 + i, 0) for i in range(max(Bs))]
    points = []
    for k, n1 in shapes:
        _, babies, giants = encdec.bsgs_split(range(k), eng.num_slots, n1)
        steps = sorted({s for s in babies + giants if s})
        keys = {s: synth.key_switch_key(eng, 100 + i, origin=f"rotation key:{s}") for i, s in enumerate(steps)}
        enc = synth.diagonals_bsgs(eng, 3, 0, range(k), n1)
        for B in Bs:
            W = [[enc if i == o else None for i in range(B)] for o in range(B)]
            forms = {"batch": lambda: eng.linear_transform_batch(cts[:B], enc, keys),
                     "loop": lambda: [eng.linear_transform(ct, enc, keys) for ct in cts[:B]],
                     "matmul": lambda: eng.lt_matmul_bsgs(W, cts[:B], keys)}
            if args.calls:
                for _ in range(args.calls):
                    forms[args.form]()
                torch.cuda.synchronize()
                continue
            a, b = forms["batch"](), forms["loop"]()      # (the batch and the loop give the same words)
            assert all(torch.equal(x.data[c][0], y.data[c][0]) for x, y in zip(a, b) for c in range(2))
            del a, b
            points.append({"preset": name, "cts": B, "k": k, "n1": n1, "keys": len(keys), "sizes": list(eng.lt_bsgs_batch_sizes),
                           **measure(forms, args.min_seconds, args.rounds)})
            print(json.dumps(points[-1]), file=sys.stderr, flush=True)
        del enc, keys
        torch.cuda.empty_cache()
    print(json.dumps(points))


def run_child(extra, seconds, wrap=()):
    cmd = ["timeout", "-k", "10", str(seconds), *wrap, sys.executable, os.path.abspath(__file__), *extra]
    return subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)


def trace(args):
    name, shape, n1 = args.trace.split(":")
    B, k = (int(v) for v in shape.lower().split("x"))
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    extra = ["--child", name, "--cts", str(B), "--shapes", f"{k}:{n1}", "--calls", str(args.calls), "--form", args.form]
    if args.sizes:
        extra += ["--sizes", args.sizes]
    r = run_child(extra, args.step_seconds, wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"))
    if r.returncode != 0:
        sys.exit(f"linear_transform_bsgs_batch: the traced run ended with status {r.returncode}")
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    if not rows:      # (a rocprofv3 that writes its database whatever format is asked for: the `kernels` view of tools/summarize_engine_ops.py)
        import sqlite3
        for path in glob.glob(os.path.join(out, "**", "*_results.db"), recursive=True):
            q = "select name, count(*), sum(end - start) from kernels group by name"
            rows += [{"Name": n, "Calls": c, "TotalDurationNs": t} for n, c, t in sqlite3.connect(path).execute(q)]
    if not rows:
        sys.exit(f"linear_transform_bsgs_batch: no kernel statistics under {out}")
    total = sum(float(r_["TotalDurationNs"]) for r_ in rows)
    result = {"point": args.trace, "form": args.form, "calls": args.calls, "unit": "us per call",
              "kernel_us_per_call": round(total / 1000 / args.calls, 1), "kernels": []}
    for r_ in sorted(rows, key=lambda r_: -float(r_["TotalDurationNs"]))[:14]:
        result["kernels"].append({"kernel": r_["Name"][:100], "launches_per_call": int(r_["Calls"]) / args.calls,
                                  "us": round(float(r_["TotalDurationNs"]) / 1000 / args.calls, 1),
                                  "share": round(float(r_["TotalDurationNs"]) / total, 4)})
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--cts", default="2,4,8,16")
    ap.add_argument("--shapes", default="64:8,16:4", help="k:n1 — k diagonals (steps 0 .. k - 1) at baby-step count n1")
    ap.add_argument("--sizes", default=None, help="group sizes of the batch for this run (default: the engine's lt_bsgs_batch_sizes)")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=420, help="time limit of each child process")
    ap.add_argument("--trace", default=None, help="preset:Bxk:n1 — one rocprofv3 kernel trace of --calls calls of that point")
    ap.add_argument("--form", default="batch", choices=("batch", "loop", "matmul"))
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("out", "lt_bsgs_batch_trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.trace:
        args.calls = args.calls or 10
        return trace(args)
    result = {"unit": "us per call (level 0, k diagonals at steps 0 .. k - 1, bsgs = n1)", "points": []}
    for name in args.presets.split(","):
        extra = ["--child", name, "--cts", args.cts, "--shapes", args.shapes, "--min-seconds", str(args.min_seconds), "--rounds",
                 str(args.rounds)]
        if args.sizes:
            extra += ["--sizes", args.sizes]
        r = run_child(extra, args.step_seconds)
        if r.returncode != 0:      # (a time limit, a fault or an abort: nothing more is started on the GPU)
            print(json.dumps(result))
            sys.exit(f"linear_transform_bsgs_batch: the run of {name} ended with status {r.returncode}")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
