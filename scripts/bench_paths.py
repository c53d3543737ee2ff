#!/usr/bin/env python
"""Cost of posterior sample paths over a grid (``sgp_grid_paths``, csrc/paths.hip).

    python scripts/bench_paths.py [--rows 1000000] [--n 500] [--reps 3] [--figures FILE]
                                  [--gpus N] [--out profiles/paths/SUMMARY.txt]

The config-3 shape: a 1000 x 1000 grid, n = 500 observations, Matern52-ARD at d = 2.  Per
m in {256, 1024, 4096} x S in {1, 16, 64}: milliseconds of the path kernel (the per-launch
hipEvents of ``sgp_profile_*``, arg-max epilogue included, ``values = NULL``), split into its
feature part and its covariance part by an m = 1 run and an n = 1 run of the same shape.  Beside
it the fp64 VALU instructions of one feature evaluation, counted in the feature loop of the
kernel's ISA with the parser of scripts/dev/isa_stats.py (``isa_counts``), and the fraction of
the fp64 VALU roof that count implies at the measured time per (row, feature).  For context the
exact ``posterior_samples_f`` at N = 8192.  ``--figures``: the error ratios that
tests/test_gpu_paths.py wrote (SGP_PATHS_FIGURES) go into the summary.  ``--gpus N`` starts N
ranks, one per GPU, each with its shard of the rows, and times the N-rank pick
(``sgp_grid_paths_comm``: the shard's kernel, the all-gather of the records, the merge) on
rank 0.
"""
import argparse, json, os, re, subprocess, sys, tempfile, time
ROOT = os.environ.get("SGP_BENCH_PACKAGE_ROOT") or \
    os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

PEAK_VALU_F64 = 78.6e12 / 2          # fp64 VALU instructions (lanes) per second: FMA = 2 flop
NOISE = 0.05 ** 2


def isa_counts(d=2):
    """fp64 VALU instructions of ONE feature evaluation in k_paths<d>, from the listing that
    scripts/dev/isa_stats.py parses.  The feature loop is what lies between the third and the
    fourth workgroup barrier of the instance (table init; the two of a feature stage; the
    covariance stage's): one iteration = one cosine per lane, its argument and the MFMA feeds.
    The library cosine reduces |arg| >= 2^30 in a block of its own (v_trig_preop); that block
    is counted apart, since no argument of this problem reaches it.  Raises when the toolchain
    or the kernel is missing: a summary without the count is not what this script is for."""
    sys.path.insert(0, os.path.join(ROOT, "scripts", "dev"))
    import isa_stats
    from safeopt_amd import build as B
    src = os.path.join(B.CSRC, "paths.hip")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "paths.s")
        r = subprocess.run([B._hipcc()] + B.BASE + B.EXTRA.get("paths.hip", []) +
                           ["-S", "--cuda-device-only", src, "-o", out],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc -S of paths.hip failed:\n" + r.stderr[-2000:])
        found = [t for name, t in isa_stats.kernels(out) if name.endswith("k_paths<%d>" % d)]
    if len(found) != 1:
        raise RuntimeError("k_paths<%d> not found in the listing of paths.hip" % d)
    stages = found[0].split("\ts_barrier")
    if len(stages) < 6:
        raise RuntimeError("k_paths<%d>: %d barriers, expected at least 5" % (d, len(stages) - 1))
    loop = stages[3]
    f64 = lambda t: len(re.findall(r"\n\tv_(?!mfma)\w+_f64", "\n" + t))
    blocks = re.split(r"\n(?=\.LBB|; %bb\.)", loop)
    large = sum(f64(b) for b in blocks if "v_trig_preop_f64" in b)
    return {"feature_loop_f64_valu": f64(loop), "large_argument_block": large,
            "per_feature": f64(loop) - large, "feature_loop_mfma": len(re.findall(r"\tv_mfma", loop)),
            "instance_f64_valu": f64(found[0]), "instance_mfma": len(re.findall(r"\tv_mfma", found[0]))}


def timed(ctx, fn, reps):
    ms = []
    for i in range(reps + 1):
        ctx.sync()
        ctx.profile_enable(True)
        fn()
        t = ctx.profile_read()[0]
        ctx.profile_enable(False)
        if i:
            ms.append(t)
    return float(np.median(ms))


def spawn(n, argv):
    """``--gpus N``: N ranks, one per GPU, in the torchrun-style environment
    ``dist.init_from_env`` reads (as scripts/swarm_optimize.py starts them); rank 0 prints."""
    import socket, subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    nonce = "%d-%x" % (os.getpid(), int(time.time() * 1e6))
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), SAFEOPT_RDZV_NONCE=nonce)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv,
                                      env=env, stdout=subprocess.PIPE if r == 0 else
                                      subprocess.DEVNULL, text=True))
    out, _ = procs[0].communicate()
    rcs = [procs[0].returncode] + [p.wait() for p in procs[1:]]
    sys.stdout.write(out)
    if any(rcs):
        sys.exit("ranks exited with %r" % (rcs,))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--figures")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.gpus > 1 and "RANK" not in os.environ:
        return spawn(a.gpus, sys.argv[1:])
    # before any GPU time: raises without toolchain or kernel (rank 0 reports: it alone counts)
    isa = isa_counts() if os.environ.get("RANK", "0") == "0" else None
    import safeopt_amd
    import safeopt_amd.gpy as gpy
    from safeopt_amd import _hip, dist, paths as P
    ctx, comm = dist.init_from_env()
    side = int(round(a.rows ** 0.5))
    grid_rows = safeopt_amd.linearly_spaced_combinations([(-5., 5.)] * 2, side)
    rng = np.random.RandomState(0)

    def model(n):
        X = rng.uniform(-5, 5, (n, 2))
        Y = (np.sin(X / [0.9, 1.5]).sum(1) + 0.05 * rng.standard_normal(n))[:, None]
        return gpy.models.GPRegression(X, Y, gpy.kern.Matern52(2, 1.7, [0.9, 1.5], ARD=True),
                                       noise_var=NOISE)
    gp, gp1 = model(a.n), model(1)
    # (every rank draws the same numbers from `rng`: the ranks hold the same GPs and paths)
    lo, hi = dist.shard_range(grid_rows.shape[0], comm.rank, comm.world)
    grid = _hip.DeviceGrid(ctx, grid_rows[lo:hi], 1, lo)

    def run(g, m, S):
        dev = g._fitted()
        desc = g.kern._desc(2)
        Om, b, W, E = P.draw_path_inputs((desc[1], desc[3]), NOISE, dev.n, 2, S, m, rng=rng)
        V = dev.path_weights(Om, b, W, E)
        return timed(ctx, lambda: grid.paths(dev, Om, b, W, V, comm=comm.world > 1), a.reps)

    rows = []
    for m in (256, 1024, 4096):
        for S in (1, 16, 64):
            rows.append({"m": m, "S": S, "ms": run(gp, m, S), "features_ms": run(gp1, m, S),
                         "covariances_ms": run(gp, 1, S)})
    if comm.rank:
        return
    # the exact draw, for context
    Xs = grid_rows[rng.permutation(grid_rows.shape[0])[:8192]]
    t0 = time.perf_counter()
    gp.posterior_samples_f(Xs, size=16)
    exact_ms = (time.perf_counter() - t0) * 1e3
    N = grid_rows.shape[0]
    lines = ["%s, %d rows (d = 2)%s, n = %d, Matern52-ARD; kernel ms (hipEvents), median of %d"
             % ("sgp_grid_paths_comm" if comm.world > 1 else "sgp_grid_paths", N,
                " over %d ranks" % comm.world if comm.world > 1 else "", a.n, a.reps),
             "    m     S   total ms  features (n = 1)  covariances (m = 1)   ns / (row feature)"]
    for r in rows:
        r["ns_per_feature"] = r["features_ms"] * 1e6 / (N * r["m"])
        lines.append("%5d %5d %10.3f %17.3f %20.3f %20.4f" % (
            r["m"], r["S"], r["ms"], r["features_ms"], r["covariances_ms"], r["ns_per_feature"]))
    lines.append("k_paths<2> feature loop, static ISA count (scripts/dev/isa_stats.py): %d fp64 VALU "
                 "instructions, of which %d in the cosine's |arg| >= 2^30 reduction, which these "
                 "arguments never enter => %d per feature evaluation (argument, reduction, both "
                 "polynomials), beside %d MFMAs (one per 16 paths); whole instance: %d fp64 VALU, %d MFMAs"
                 % (isa["feature_loop_f64_valu"], isa["large_argument_block"], isa["per_feature"],
                    isa["feature_loop_mfma"], isa["instance_f64_valu"], isa["instance_mfma"]))
    roof_ns = isa["per_feature"] * 1e9 / PEAK_VALU_F64
    lines.append("fp64 VALU roof: %.1f T lane-instructions / s => %.5f ns per (row, feature) at %d "
                 "instructions" % (PEAK_VALU_F64 / 1e12, roof_ns, isa["per_feature"]))
    lines.append("    m     S   ns / (row feature)   fraction of the fp64 VALU roof")
    for r in rows:
        r["valu_roof_fraction"] = roof_ns / r["ns_per_feature"]
        lines.append("%5d %5d %20.4f %32.3f" % (r["m"], r["S"], r["ns_per_feature"],
                                                r["valu_roof_fraction"]))
    lines.append("exact posterior_samples_f, N = 8192, 16 samples, n = %d: %.1f ms (host clock, one call)"
                 % (a.n, exact_ms))
    fig = {}
    if a.figures and os.path.exists(a.figures):
        for ln in open(a.figures):
            k, v = ln.split()
            fig[k] = max(fig.get(k, 0.0), float(v))
        lines.append("tests/test_gpu_paths.py, worst observed over its cases: weights residual / bound "
                     "= %.3f; evaluation |dev - ref| / (c budget) = %.3f (|dev - ref| / budget = %.2e)"
                     % (fig.get("weights", float("nan")), fig.get("evaluation", float("nan")),
                        fig.get("evaluation_abs", float("nan"))))
    else:
        lines.append("error ratios of tests/test_gpu_paths.py: not measured (no --figures file)")
    line = json.dumps({"bench": "paths", "gpus": comm.world, "rows": rows, "isa": isa, "exact_8192_ms": exact_ms,
                       "figures": fig})
    print(line)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n" + line + "\n")


if __name__ == "__main__":
    main()
