"""linear_transform_batch against the loop of linear_transform it replaces, on one GPU:
    python tools/linear_transform_batch.py [--presets silver,gold] [--cts 2,4,8,16] [--ks 8,16] [--min-seconds 0.3] [--rounds 5]
For every preset at level 0 and every (B, k) of --cts x --ks, B ciphertexts under k rotated diagonals + the step-0 one:
    batch    linear_transform_batch(cts, diags, keys)     groups of 4 and 2: every key and diagonal read once per group
    loop     [linear_transform(ct, diags, keys) for ct in cts]
Each preset is measured in a child process of its own under `timeout -k 10` (--step-seconds); a child that fails ends the run.
Inside a child the two forms of a point are timed alternately with device events after a warm-up of each, every timing over at
least --min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median
over its rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratio
loop / batch and whether the batch wins by more than the two spreads combined.
    python tools/linear_transform_batch.py --trace gold:8x8 [--calls 10] [--out out/lt_batch_trace]
runs one `rocprofv3 --kernel-trace --stats` pass over --calls batch calls of that point (preset:BxK) in a process of its own, the
program after `--`, under `timeout -k 10`, and prints the kernels' totals from its statistics: for ks_inner_ltb_kernel also the
time per (ciphertext, key) and, at gold, the HBM rate that time means at the 281 MB (1 key x 4 ciphertexts) and the 189 MB (digits shared
between two keys) of DESIGN.md 4.2.  Synthetic keys and ciphertexts (utils/synth.py): the kernels do not look at the values."""
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
    out["batch_wins"] = bool(med["loop"] / med["batch"] > 1 + spread["loop"] + spread["batch"])
    return out


def child(args):
    """one preset (or one point of it, --calls times, for a trace) in this process"""
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("linear_transform_batch: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    name = args.child
    shapes = [(int(b), int(k)) for b in args.cts.split(",") for k in args.ks.split(",")]
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and hasattr(eng.backend, "linear_transform_batch_native")
    kmax, bmax = max(k for _, k in shapes), max(b for b, _ in shapes)
    keys = [synth.key_switch_key(eng, 100 + i, origin=f"rotation key:{i + 1}") for i in range(kmax)]
    cts = [synth.ciphertext(eng, 7 + i, 0) for i in range(bmax)]
    points = []
    for k in sorted({k for _, k in shapes}):
        enc = synth.diagonals(eng, 3, 0, range(k + 1))
        for B in sorted({b for b, kk in shapes if kk == k}):
            forms = {"batch": lambda: eng.linear_transform_batch(cts[:B], enc, keys[:k]),
                     "loop": lambda: [eng.linear_transform(ct, enc, keys[:k]) for ct in cts[:B]]}
            if args.calls:
                for _ in range(args.calls):
                    forms["batch"]()
                torch.cuda.synchronize()
                continue
            a, b = forms["batch"](), forms["loop"]()      # (the timed forms give the same words)
            assert all(torch.equal(x.data[c][0], y.data[c][0]) for x, y in zip(a, b) for c in range(2))
            del a, b
            points.append({"preset": name, "cts": B, "k": k, **measure(forms, args.min_seconds, args.rounds)})
            print(json.dumps(points[-1]), file=sys.stderr, flush=True)
        del enc
    print(json.dumps(points))


def run_child(extra, seconds, wrap=()):
    cmd = ["timeout", "-k", "10", str(seconds), *wrap, sys.executable, os.path.abspath(__file__), *extra]
    return subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)


def trace(args):
    name, shape = args.trace.split(":")
    B, k = (int(v) for v in shape.lower().split("x"))
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    r = run_child(["--child", name, "--cts", str(B), "--ks", str(k), "--calls", str(args.calls)], args.step_seconds,
                  wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--"))
    if r.returncode != 0:
        sys.exit(f"linear_transform_batch: the traced run ended with status {r.returncode}")
    rows = []
    for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    if not rows:      # (a rocprofv3 that writes its database whatever format is asked for: the `kernels` view of tools/summarize_engine_ops.py)
        import sqlite3
        for path in glob.glob(os.path.join(out, "**", "*_results.db"), recursive=True):
            q = "select name, count(*), sum(end - start) from kernels group by name"
            rows += [{"Name": n, "Calls": c, "TotalDurationNs": t} for n, c, t in sqlite3.connect(path).execute(q)]
    if not rows:
        sys.exit(f"linear_transform_batch: no kernel statistics under {out}")
    total = sum(float(r_["TotalDurationNs"]) for r_ in rows)
    result = {"point": args.trace, "calls": args.calls, "unit": "us per call", "kernels": []}
    for r_ in sorted(rows, key=lambda r_: -float(r_["TotalDurationNs"]))[:12]:
        us = float(r_["TotalDurationNs"]) / 1000 / args.calls
        row = {"kernel": r_["Name"][:100], "launches_per_call": int(r_["Calls"]) / args.calls, "us": round(us, 1),
               "share": round(float(r_["TotalDurationNs"]) / total, 4)}
        if "ks_inner_ltb_kernel" in r_["Name"]:
            groups = B - B % 2                        # ciphertexts that go through the batched kernel (a lone last one does not)
            per = us / (groups * k)
            row["us_per_ct_key"] = round(per, 2)
            if name == "gold":                        # (the byte counts of DESIGN.md 4.2 are gold's at level 0)
                row.update({"TBps_if_281MB": round(281e6 / per / 1e6, 2), "TBps_if_189MB": round(189e6 / per / 1e6, 2)})
        result["kernels"].append(row)
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--cts", default="2,4,8,16")
    ap.add_argument("--ks", default="8,16")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=420, help="time limit of each child process")
    ap.add_argument("--trace", default=None, help="preset:BxK — one rocprofv3 kernel trace of --calls batch calls of that point")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--out", default=os.path.join("out", "lt_batch_trace"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.trace:
        args.calls = args.calls or 10
        return trace(args)
    result = {"unit": "us per call (level 0, k rotated diagonals + step 0)", "points": []}
    for name in args.presets.split(","):
        r = run_child(["--child", name, "--cts", args.cts, "--ks", args.ks, "--min-seconds", str(args.min_seconds), "--rounds",
                       str(args.rounds)], args.step_seconds)
        if r.returncode != 0:      # (a time limit, a fault or an abort: nothing more is started on the GPU)
            print(json.dumps(result))
            sys.exit(f"linear_transform_batch: the run of {name} ended with status {r.returncode}")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
