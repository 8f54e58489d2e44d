"""mod_raise / mod_raise_batch against the torch chain that defines their words, on one GPU:
    python tools/mod_raise.py [--presets silver,gold] [--cts 8] [--min-seconds 0.3] [--rounds 5]
For every preset, operands at the last level (two rows: the shape a bootstrap raises from):
    mod_raise        mod_raise(ct)
    mod_raise_batch  mod_raise_batch(B ciphertexts) for every B of --cts
each in two forms on the SAME engine:
    native   one native call (lf_mod_raise)
    chain    the engine's switch mod_raise_native off: torch.remainder / torch.where on the same device, the definition, which is
             what a sharded or multi-device engine runs on each device
Each preset is measured in a child process of its own under `timeout -k 10` (--step-seconds); a child that fails ends the run.
The two forms of a point are timed alternately with device events after a warm-up of each, every timing over at least
--min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its
rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratio chain / native,
whether the native form wins by more than the two spreads combined, and the bytes the native call moves over its time (16 read
and 16 * rows written per coefficient and ciphertext).  Synthetic ciphertexts (utils/synth.py): the kernel does not look at
the values."""
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
    spread = {f: (max(t) - min(t)) / med[f] for f, t in times.items()}
    out = {f: round(med[f], 1) for f in forms}
    out.update({f"spread_{f}": round(s, 4) for f, s in spread.items()})
    out["chain_over_native"] = round(med["chain"] / med["native"], 3)
    out["native_wins"] = bool(med["chain"] / med["native"] > 1 + spread["chain"] + spread["native"])
    out["native_loses"] = bool(med["native"] / med["chain"] > 1 + spread["chain"] + spread["native"])
    return out


def child(args):
    """one preset in this process"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("mod_raise: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    name = args.child
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    top = eng.num_levels - 1
    N, rows = eng.ctx.N, eng._rows(0, 0, False)
    bmax = max(int(b) for b in args.cts.split(","))
    cts = [synth.ciphertext(eng, 7 + i, top) for i in range(bmax)]
    assert eng._mod_raise_device(cts[0]) == 0
    same = lambda a, b: all(torch.equal(x.data[c][0], y.data[c][0]) for x, y in zip(a, b) for c in range(2))
    points = []

    def point(tag, fn, count):
        def chain():
            eng.mod_raise_native = False
            try:
                return fn()
            finally:
                eng.mod_raise_native = True
        a, b = fn(), chain()
        assert same(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b])      # (the timed forms give the same words)
        m = measure({"native": fn, "chain": chain}, args.min_seconds, args.rounds)
        moved = count * N * 16 * (1 + rows)
        points.append({"preset": name, "rows": rows, **tag, **m, "native_bytes": moved, "native_GBps": round(moved / m["native"] / 1e3, 1),
                       "chain_GBps": round(moved / m["chain"] / 1e3, 1)})
        print(json.dumps(points[-1]), file=sys.stderr, flush=True)

    point({"op": "mod_raise"}, lambda: eng.mod_raise(cts[0]), 1)
    for B in sorted(int(b) for b in args.cts.split(",")):
        point({"op": "mod_raise_batch", "cts": B}, lambda: eng.mod_raise_batch(cts[:B]), B)
    print(json.dumps(points))


def run_child(extra, seconds):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), *extra]
    return subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--cts", default="8")
    ap.add_argument("--min-seconds", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-seconds", type=int, default=300, help="time limit of each child process")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    result = {"unit": "us per call", "points": []}
    for name in args.presets.split(","):
        r = run_child(["--child", name, "--cts", args.cts, "--min-seconds", str(args.min_seconds), "--rounds", str(args.rounds)],
                      args.step_seconds)
        if r.returncode != 0:      # (a time limit, a fault or an abort: nothing more is started on the GPU)
            print(json.dumps(result))
            sys.exit(f"mod_raise: the run of {name} ended with status {r.returncode}")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
