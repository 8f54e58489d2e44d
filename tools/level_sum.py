"""level_sum / level_up / level_up_batch against the compositions that define them, on one GPU:
    python tools/level_sum.py [--presets silver,gold] [--cts 2,4,8,16] [--min-seconds 0.3] [--rounds 5]
For every preset, operands at levels 0 .. 4:
    level_up        level_up(ct, 1) and level_up(ct, 4)                                     across 1 and 4 levels
    level_up_batch  level_up_batch(B ciphertexts, 1) for every B of --cts
    cheb_square     level_sum([(sq, 2)], const=-1)                 = add_scalar(mult_int_scalar(sq, 2), -1)
    cheb_product    level_sum([(prod, 2), (p, -1)]), p one level up = auto_cc_sub(mult_int_scalar(prod, 2), p)
    residual        level_sum of four terms over three levels (0, 1, 1, 2), weights 1, 1, -1, 3
each in two forms on the SAME engine:
    native       one native call (lf_level_sum)
    composition  the engine's switch level_sum_native off: the reference's element-wise chains (rescale, slices, mont_enter_scalar,
                 reduce_2q, mont_add), which is what runs wherever the native call does not apply
Each preset is measured in a child process of its own under `timeout -k 10` (--step-seconds); a child that fails ends the run.
The two forms of a point are timed alternately with device events after a warm-up of each, every timing over at least
--min-seconds of work, --rounds rounds; the median is kept and every form's own run-to-run spread ((max - min) / median over its
rounds) is reported beside it.  Prints one JSON line: microseconds per call for each form, the spreads, the ratio composition /
native, whether the native form wins by more than the two spreads combined, and the bytes the native call moves over its time.
Synthetic ciphertexts (utils/synth.py): the kernel does not look at the values."""
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
    out["composition_over_native"] = round(med["composition"] / med["native"], 3)
    out["native_wins"] = bool(med["composition"] / med["native"] > 1 + spread["composition"] + spread["native"])
    out["native_loses"] = bool(med["native"] / med["composition"] > 1 + spread["composition"] + spread["native"])
    return out


def child(args):
    """one preset in this process"""
    import torch
    if not torch.cuda.is_available():
        sys.exit("level_sum: no GPU")
    import __graft_entry__ as g
    g.build()
    from liberate_fhe_amd.fhe import ckks_engine, presets
    from liberate_fhe_amd.utils import synth
    name = args.child
    params = {k: v for k, v in presets.params[name].items() if k != "devices"}
    eng = ckks_engine(devices=["cuda:0"], **params)
    assert eng._native_level(0) is not None and hasattr(eng.backend, "level_sum_call") and eng.num_levels > 5
    N = eng.ctx.N
    rows = lambda level: eng._rows(0, level, False)
    bmax = max(int(b) for b in args.cts.split(","))
    at = {l: [synth.ciphertext(eng, 7 + 10 * l + i, l) for i in range(bmax if l == 0 else 2)] for l in range(3)}
    same = lambda a, b: all(torch.equal(x.data[c][0], y.data[c][0]) for x, y in zip(a, b) for c in range(2))
    points = []

    def point(tag, fn, bytes_moved):
        def composition():
            eng.level_sum_native = False
            try:
                return fn()
            finally:
                eng.level_sum_native = True
        a, b = fn(), composition()
        assert same(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b])      # (the timed forms give the same words)
        m = measure({"native": fn, "composition": composition}, args.min_seconds, args.rounds)
        points.append({"preset": name, **tag, **m, "native_bytes": bytes_moved, "native_GBps": round(bytes_moved / m["native"] / 1e3, 1)})
        print(json.dumps(points[-1]), file=sys.stderr, flush=True)

    # bytes of a native call, both components: per levelled term the surviving rows and the dropped row, per same-level term
    # its rows, and the output rows
    moved = lambda L, levelled, level_terms, sets=1: 2 * 8 * N * sets * (levelled * (rows(L) + 1) + level_terms * rows(L) + rows(L))
    point({"op": "level_up", "levels": 1}, lambda: eng.level_up(at[0][0], 1), moved(1, 1, 0))
    point({"op": "level_up", "levels": 4}, lambda: eng.level_up(at[0][0], 4), moved(4, 1, 0))
    for B in sorted(int(b) for b in args.cts.split(",")):
        point({"op": "level_up_batch", "cts": B}, lambda: eng.level_up_batch(at[0][:B], 1), moved(1, 1, 0, B))
    point({"op": "cheb_square"}, lambda: eng.level_sum([(at[1][0], 2)], const=-1), moved(1, 0, 1))
    point({"op": "cheb_product"}, lambda: eng.level_sum([(at[1][0], 2), (at[0][0], -1)]), moved(1, 1, 1))
    point({"op": "residual", "terms": 4, "levels": 3},
          lambda: eng.level_sum([(at[2][0], 1), (at[0][0], 1), (at[1][0], -1), (at[1][1], 3)]), moved(2, 3, 1))
    print(json.dumps(points))


def run_child(extra, seconds):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__), *extra]
    return subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", default="silver,gold")
    ap.add_argument("--cts", default="2,4,8,16")
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
            sys.exit(f"level_sum: the run of {name} ended with status {r.returncode}")
        result["points"] += json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(result))


if __name__ == "__main__":
    main()
