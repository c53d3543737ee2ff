"""The long-double reference of the incremental-path tests and their case table, checked
without a GPU: (a) the reference is right to its own precision, (b) the float64 oracle --
an implementation with the device's number format -- stays within 1 % of every tolerance the
GPU module uses, so those tolerances measure the kernels and not the data, (c) every rank-1
case moves mean and variance by far more than the tolerances, so a wrong update vector, a
wrong staged row or a skipped block of 16 cannot hide below them, (d) the rows whose safe-set
membership is too close to call are few and both memberships are compared."""
import numpy as np
import pytest

import _incremental_ref as R
from _gpu_common import MEAN_TOL, VAR_TOL
from oracle import gp_numpy as gpn

MARGIN = 0.01
LINV_TOL = ALPHA_TOL = Q_TOL = 1e-8         # the GPU module's bounds (tests/test_gpu_incremental.py)


def _oracle(spec, X, Y):
    return gpn.GPRegression(X, np.asarray(Y)[:, None], R.make_kernel(gpn, spec), noise_var=R.NOISE)


def _posterior_margin(go, rows, ref_mean, ref_var, kd, what):
    m, v = go.predict_noiseless(rows)
    m, v = m[:, 0], v[:, 0]
    em = np.max(np.abs(m - ref_mean)) / max(np.max(np.abs(ref_mean)), 1e-300)
    ev = np.max(np.abs(v - ref_var)) / kd
    big = ref_var > 1e-6 * kd
    er = np.max(np.abs(v[big] - ref_var[big]) / ref_var[big]) if big.any() else 0.0
    print("%s: mean %.2e  var %.2e  var (relative) %.2e" % (what, em, ev, er))
    assert em < MARGIN * MEAN_TOL, what
    assert ev < MARGIN * VAR_TOL, what
    assert er < MARGIN * 1e-5, what
    return m, v


def _factor_margin(go, snap, what):
    alpha = go.woodbury_vector.ravel()
    ea = np.max(np.abs(alpha - snap["alpha"])) / np.max(np.abs(snap["alpha"]))
    print("%s: alpha %.2e" % (what, ea))
    assert ea < MARGIN * ALPHA_TOL, what
    if "Linv" in snap:
        el = np.max(np.abs(np.linalg.inv(go.L) - snap["Linv"]))
        print("%s: L^-1 %.2e" % (what, el))
        assert el < MARGIN * LINV_TOL, what


# ---- (a) the reference --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rbf_d1_16", "mat32_d3_32", "prod_d3_128"])
def test_reference_factor_inverts_ky(name):
    """L^-1 Ky L^-T = I to 1e-17 cond(Ky) -- on a factor that was fitted and then grown row by
    row, which is how every reference of the GPU module comes about."""
    spec, d, n_fit, n_end = R.APPEND_CASES[name]
    X, Y, _, _, _ = R.data(name, d, n_end)
    gp = R.RefGP(spec, X[:n_fit], Y[:n_fit])
    for i in range(n_fit, n_end):
        gp.append(X[i], Y[i])
    Ky, Li = gp.Ky(), gp.Linv()
    cond = np.linalg.cond(R.f64(Ky))
    err = float(np.max(np.abs(Li @ Ky @ Li.T - np.eye(gp.n, dtype=R.LD))))
    print("%s: |L^-1 Ky L^-T - I| = %.2e, cond = %.2e" % (name, err, cond))
    assert err <= 1e-17 * cond
    # ... and it is the factor of a fit at n_end
    assert float(np.max(np.abs(R.cholesky(Ky) - gp.L))) <= 1e-17 * cond


@pytest.mark.parametrize("name", ["g1_mat32_d2_N15", "g3_mixed_d3_N197", "chain_aaa_011"])
def test_reference_closed_form_equals_its_refit(name):
    """The closed-form refresh, in long double, against the refit: 1e-16 cond(Ky)."""
    ref = R.rank1_reference(name)
    case = R.RANK1_CASES[name]
    st = ref["steps"][0]
    for g, (cm, cv) in st["closed"].items():
        gp = R.RefGP(case["gps"][g][0], ref["X"][g], ref["Y"][g])
        cond = np.linalg.cond(R.f64(gp.Ky()))
        em = float(np.max(np.abs(cm - st["mean_ld"][g])))
        ev = float(np.max(np.abs(cv - st["var_ld"][g])))
        print("%s GP %d: mean %.2e var %.2e, cond = %.2e" % (name, g, em, ev, cond))
        assert em <= 1e-16 * cond and ev <= 1e-16 * cond


# ---- (b) margin -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.APPEND_CASES))
def test_margin_append_cases(name):
    spec, d, n_fit, n_end = R.APPEND_CASES[name]
    X, Y, Xs, _, _ = R.data(name, d, n_end)
    for snap in R.append_reference(name):
        n = snap["n"]
        go = _oracle(spec, X[:n], Y[:n])
        what = "%s n = %d" % (name, n)
        _posterior_margin(go, Xs, snap["mean"], snap["var"], R.kdiag(spec), what)
        _factor_margin(go, snap, what)


@pytest.mark.parametrize("name", sorted(R.POP_CASES))
def test_margin_pop_cases(name):
    spec, d, n = R.POP_CASES[name]
    Xs = R.data(name, d, n, extra=5)[2]
    for i, (what, snap) in enumerate(R.pop_reference(name)):
        go = _oracle(spec, snap["X"], snap["Y"])
        what = "%s call %d (%s) n = %d" % (name, i, what, snap["n"])
        _posterior_margin(go, Xs, snap["mean"], snap["var"], R.kdiag(spec), what)
        _factor_margin(go, snap, what)


def test_margin_capacity_case():
    spec, d, n0, n_end = R.CAPACITY
    Xs = R.data("capacity", d, n_end)[2]
    ref = R.capacity_reference()
    assert sorted(ref) == sorted(R.CAPACITY_CHECK)
    for n, snap in sorted(ref.items()):
        go = _oracle(spec, snap["X"], snap["Y"])
        _posterior_margin(go, Xs, snap["mean"], snap["var"], R.kdiag(spec), "capacity n = %d" % n)
        _factor_margin(go, snap, "capacity n = %d" % n)


@pytest.mark.parametrize("name", sorted(R.RANK1_CASES))
def test_margin_rank1_cases(name):
    case, ref = R.RANK1_CASES[name], R.rank1_reference(name)
    G = len(case["gps"])
    X, Y = [x.copy() for x in ref["X"]], [y.copy() for y in ref["Y"]]
    for t, st in enumerate(ref["steps"]):
        for g in range(G):
            if case["which"][g]:
                X[g] = np.vstack([X[g], st["xstar"][None, :]])
                Y[g] = np.append(Y[g], st["ystar"][g])
            go = _oracle(case["gps"][g][0], X[g], Y[g])
            what = "%s step %d GP %d" % (name, t, g)
            m, v = _posterior_margin(go, ref["pts"], st["mean"][g], st["var"][g],
                                     ref["kdiag"][g], what)
            sd = np.sqrt(v)
            q = np.stack([m - st["beta"] * sd, m + st["beta"] * sd], axis=1)
            eq = np.max(np.abs(q - st["Q"][:, 2 * g:2 * g + 2]))
            print("%s: Q %.2e" % (what, eq))
            assert eq < MARGIN * Q_TOL, what


def test_margin_context_switch():
    case, ref, sw = R.RANK1_CASES["ctx_prod_d3"], R.rank1_reference("ctx_prod_d3"), R.context_switch_reference()
    st = ref["steps"][0]
    for g, (spec, _, _) in enumerate(case["gps"]):
        X = np.vstack([ref["X"][g], st["xstar"][None, :], sw["x2"][None, :]])
        Y = np.r_[ref["Y"][g], st["ystar"][g], sw["y2"][g]]
        m, v = _posterior_margin(_oracle(spec, X, Y), sw["pts"], sw["mean"][g], sw["var"][g],
                                 ref["kdiag"][g], "context switch GP %d" % g)
        sd = np.sqrt(v)
        q = np.stack([m - sw["beta"] * sd, m + sw["beta"] * sd], axis=1)
        assert np.max(np.abs(q - sw["Q"][:, 2 * g:2 * g + 2])) < MARGIN * Q_TOL
    # the new context matters: the old context's posterior is far from this one
    assert np.max(np.abs(sw["mean"] - st["mean"])) > 1e-2
    assert not sw["excluded"].any()


# ---- (c) sensitivity ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.RANK1_CASES))
def test_rank1_cases_move_the_posterior(name):
    case, ref = R.RANK1_CASES[name], R.rank1_reference(name)
    mean0, var0 = ref["before"]
    for t, st in enumerate(ref["steps"]):
        for g in range(len(case["gps"])):
            if not case["which"][g]:
                assert np.array_equal(st["mean"][g], mean0[g])      # untouched by the step
                continue
            kd = ref["kdiag"][g]
            dm = np.max(np.abs(st["mean"][g] - mean0[g])) / np.max(np.abs(st["mean"][g]))
            dv = np.max(var0[g] - st["var"][g]) / kd
            print("%s step %d GP %d: mean moves %.2e, w^T k %.2e, var drops %.2e"
                  % (name, t, g, dm, st["wk"][g], dv))
            assert dm >= 1e-2
            assert st["wk"][g] >= 0.1
            assert dv >= 1e-3
        mean0, var0 = st["mean"], st["var"]


def test_append_case_1024_reaches_alpha_beyond_1024():
    """The append 1025 -> 1026 is the only one whose update of alpha has an entry at
    j >= 1024 (k_append_finish walks alpha with 1024 threads): that entry, w_j r / s^2, must be
    a good part of max |alpha| and show in the mean at a test row, or an error there of one
    part in a million -- one hundred times the tolerance on alpha -- would pass."""
    name = "rbf_d2_1024"
    spec, d, n_fit, n_end = R.APPEND_CASES[name]
    X, Y, Xs, _, _ = R.data(name, d, n_end)
    gp = R.RefGP(spec, X[:n_end - 1], Y[:n_end - 1])
    a0 = gp.alpha()
    gp.append(X[n_end - 1], Y[n_end - 1])
    a1 = gp.alpha()
    move = float(abs(a1[1024] - a0[1024]) / np.max(np.abs(a1)))
    m = gp.predict(Xs)[0]
    k = float(np.max(R.kern(spec, Xs, X[1024:1025])))
    in_mean = float(abs(a1[1024] - a0[1024]) * k / np.max(np.abs(m)))
    print("alpha[1024] moves by %.3f max|alpha|, the mean by %.3f max|mean|" % (move, in_mean))
    assert move >= 0.05 and in_mean >= 0.01


# ---- (d) rows whose safe-set membership is not compared ----------------------------------------
@pytest.mark.parametrize("name", sorted(R.RANK1_CASES))
def test_rank1_cases_compare_both_values_of_S(name):
    case, ref = R.RANK1_CASES[name], R.rank1_reference(name)
    N = case["N"]
    for t, st in enumerate(ref["steps"]):
        n_ex = int(st["excluded"].sum())
        kept = st["S"][~st["excluded"]]
        print("%s step %d: %d of %d rows excluded, %d safe" % (name, t, n_ex, N, kept.sum()))
        assert n_ex <= 0.01 * N
        if N < 100:
            assert n_ex == 0
        if N > 1:
            assert kept.any() and not kept.all()
        else:
            assert bool(kept[0]) == case["safe"]      # (the two one-row cases: one value each)
        assert st["ret"][1] == bool(st["S"].any())


def test_every_kernel_instance_and_row_count_is_in_the_table():
    ds = {c["d"] for c in R.RANK1_CASES.values()}
    assert {1, 2, 3, 4, 5, 8} <= ds
    assert {1, 15, 64, 197, 4099} <= {c["N"] for c in R.RANK1_CASES.values()}
    kinds = {p[0] for c in R.RANK1_CASES.values() for spec, _, _ in c["gps"] for p in spec}
    assert kinds == {"RBF", "Matern32", "Matern52"}
    # both sides of k_rank1's LDS switch, n_pad (d + 1) <= 6144 doubles
    pads = [(-(-(n + t) // 16) * 16) * (c["d"] + 1) for c in R.RANK1_CASES.values()
            for _, _, n in c["gps"] for t in range(1, c["steps"] + 1)]
    assert min(pads) <= 6144 < max(pads)
