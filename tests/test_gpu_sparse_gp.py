"""Sparse GP regression on the device (do_sparse_gp / sr_gp_fit_sparse) against the long-double evaluation of the DTC
formulas (tests/_sparse_ref.py), and every posterior consumer on a sparse model against the existing oracle functions
evaluated with beta := woodbury_vector, inv_K := woodbury_inv.

Tolerances.  Consumers of a model GIVEN alpha and Wt: the project's written ones.  The fit: per case
e_ref = |fp64 NumPy restatement - long-double truth| (long double for every case: m <= 300), and the device must be within
max(project tolerance, 10 e_ref) of the truth; each case asserts cond K_uu <= 1e6 and e_ref(var) <= 1e-10 sigma_f^2 first.
The ratios device error / e_ref are printed by every case (pytest -s) and recorded in profiles/r09_sparse_fit.txt.  Worst
measured: 45.5 (M of the m = 1 case: 2.3e-16 absolute against e_ref = 5e-18, inside the relative 1e-10); worst among the
cases whose e_ref exceeds 1e-13: 13.7 (M, mat52, 2.7e-10 absolute, inside 1e-10 |M|) and 10.6 (mu of rbf-2-3-96-3000: 1.4e-10
against the project's 8e-10); every other ratio is below 10, the variance's below 3."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

import _sparse_ref as R
from _helpers import mu_atol
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

JIT = 1e-6
# (kernel, n_out, D, m, N, chunk): every kernel identifier, n_out in {1, 2, 4}, D in {2, 3, 5}, m in {1, 96, 128, 129, 300},
# N in {m, m + 1, 3000, 70001}; chunk small enough that N = 70001 spans 18 chunks and a ragged last one
CASES = [("rbf", 2, 3, 96, 3000, None), ("rbf", 1, 2, 1, 1, None), ("rbf", 1, 2, 1, 2, None), ("rbf", 2, 2, 96, 96, None),
         ("rbf", 1, 2, 96, 97, None), ("rbf", 2, 3, 128, 129, None), ("rbf", 2, 3, 128, 3000, 1000),
         ("rbf", 4, 5, 129, 3000, None), ("rbf", 2, 5, 300, 3000, 512), ("rbf", 2, 3, 96, 70001, 4096),
         ("mat52", 2, 3, 96, 3000, None), ("mat52", 4, 5, 129, 130, None), ("lin_rbf", 2, 2, 12, 3000, None),
         ("lin_mat52", 1, 3, 24, 3000, 100), ("lin_mat52", 2, 3, 24, 70001, 4096)]


def _sparse_model(case, chunk=None, Z=True):
    from safe_exploration_amd import SimpleGPModel
    kt, n_out, D = case["kern_types"], len(case["kern_types"]), case["X"].shape[1]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=kt, hyp=case["hyp"])
    gp.do_sparse_gp = True
    if chunk is not None:
        gp.set_sparse_chunk(chunk)
    gp.train(case["X"], case["Y"], case["Zu"].shape[0], opt_hyp=False, Z=case["Zu"] if Z else None)
    return gp


def _truth(case):
    a = (case["kern_types"], case["hyp"], case["Zu"], case["X"], case["Y"], case["s2"], JIT)
    b_np, M_np, cond = R.sparse_fit_np(*a)
    b_ld, M_ld = R.sparse_fit_ld(*a)
    return b_np, M_np, cond, b_ld, M_ld


@pytest.mark.parametrize("spec", CASES, ids=lambda s: "-".join(str(v) for v in s))
def test_sparse_fit_matches_long_double_truth(spec):
    kern, n_out, D, m, N, chunk = spec
    assert np.finfo(np.longdouble).eps < 1e-18, "the truth needs an extended long double"
    case = R.make_case(100 + m + N % 1000, kern, n_out, D, m, N)
    kt, hyp, Zu, xq = case["kern_types"], case["hyp"], case["Zu"], case["xq"]
    b_np, M_np, cond, b_ld, M_ld = _truth(case)
    sf2 = R.sigma_f2(kt, hyp, xq)
    mu_np, var_np = R.predict_any(kt, hyp, Zu, b_np, M_np, xq)
    mu_ld, var_ld = R.predict_any(kt, hyp, Zu, b_ld, M_ld, xq, ld=True)
    e_beta = float(np.abs(b_np - b_ld).max())
    e_M = max(float(np.abs(a - b).max()) for a, b in zip(M_np, M_ld))
    e_mu = float(np.abs(mu_np - mu_ld).max())
    e_var = float((np.abs(var_np - var_ld) / sf2).max())
    jac_t = orc.gp_mean_jacobian_k(xq, Zu, b_ld.astype(np.float64), kt, hyp)
    e_jac = float(np.abs(orc.gp_mean_jacobian_k(xq, Zu, b_np, kt, hyp) - jac_t).max())
    # an uninformative case fails instead of passing loosely
    assert max(cond) <= 1e6, cond
    assert e_var <= 1e-10, e_var
    assert float(var_ld.min()) > 1e-6          # no query sits on the variance clip

    gp = _sparse_model(case, chunk)
    assert gp.is_sparse and gp.z.shape == (m, D) and gp.x_train.shape == (N, D)
    beta, inv_K = gp.beta, gp.inv_K
    mu, var, jac = gp.predict(xq, compute_gradients=True)
    scale = float(np.sqrt(sf2.max()) * np.abs(b_ld.astype(np.float64)).sum(0).max())      # sigma_f |beta|_1 (_helpers.mu_atol)
    d_beta = float(np.abs(beta - b_ld).max())
    d_M = max(float(np.abs(a - b).max()) for a, b in zip(inv_K, M_ld))
    d_mu = float(np.abs(mu - mu_ld).max())
    d_var = float((np.abs(var - var_ld) / sf2).max())
    d_jac = float(np.abs(jac - jac_t).max())
    tiny = 1e-300
    print("sparse-fit %s cond %.1e | device error / e_ref: beta %.2f (%.1e) M %.2f (%.1e) mu %.2f (%.1e) var %.2f (%.1e) jac %.2f (%.1e)"
          % (spec, max(cond), d_beta / max(e_beta, tiny), e_beta, d_M / max(e_M, tiny), e_M, d_mu / max(e_mu, tiny), e_mu,
             d_var / max(e_var, tiny), e_var, d_jac / max(e_jac, tiny), e_jac))
    # project tolerances: mu, J rtol 1e-10 / atol 1e-12 sigma_f |beta|_1; var atol 1e-9 sigma_f^2; beta, M: 1e-10 relative
    assert d_mu <= max(1e-10 * float(np.abs(mu_ld).max()) + 1e-12 * scale, 10 * e_mu)
    ls_min = float(min(np.min(v) for h in hyp for k, v in h.items() if "lengthscale" in k))
    assert d_jac <= max(1e-10 * float(np.abs(jac_t).max()) + 1e-12 * scale / ls_min, 10 * e_jac)
    assert d_var <= max(1e-9, 10 * e_var)
    assert d_beta <= max(1e-10 * float(np.abs(b_ld).max()), 10 * e_beta)
    assert d_M <= max(1e-10 * max(float(np.abs(a).max()) for a in M_ld), 10 * e_M)
    for d in range(n_out):
        assert np.array_equal(inv_K[d], inv_K[d].T) or np.abs(inv_K[d] - inv_K[d].T).max() <= 1e-12 * np.abs(inv_K[d]).max()


def _headline():
    return R.make_case(5, "rbf", 2, 3, 96, 3000)


def test_sparse_differs_from_subset_of_data_and_matches_the_sparse_oracle():
    """FAILS without the feature: on the parent commit do_sparse_gp is ignored and the model is the subset-of-data one."""
    from safe_exploration_amd import SimpleGPModel
    case = _headline()
    kt, hyp, Zu, xq = case["kern_types"], case["hyp"], case["Zu"], case["xq"]
    b_np, M_np, cond, b_ld, M_ld = _truth(case)
    mu_ld, var_ld = R.predict_any(kt, hyp, Zu, b_ld, M_ld, xq, ld=True)
    mu_np, var_np = R.predict_any(kt, hyp, Zu, b_np, M_np, xq)
    gp = _sparse_model(case)
    mu, var = gp.predict(xq)
    sod = SimpleGPModel(2, 2, 1, kern_types=kt, hyp=hyp)
    idx = np.array([int(np.where((case["X"] == z).all(1))[0][0]) for z in Zu])
    sod.train(Zu, case["Y"][idx], opt_hyp=False)
    mu_s, var_s = sod.predict(xq)
    assert np.abs(mu - mu_s).max() > 1e-3 and np.abs(var - var_s).max() > 1e-4      # far beyond any tolerance
    sf2 = R.sigma_f2(kt, hyp, xq)
    assert np.abs(mu - mu_ld).max() <= max(1e-10 * np.abs(mu_ld).max() + mu_atol(dict(signal_var=sf2, beta=b_np)),
                                           10 * np.abs(mu_np - mu_ld).max())
    assert (np.abs(var - var_ld) / sf2).max() <= max(1e-9, 10 * (np.abs(var_np - var_ld) / sf2).max())


def test_posterior_consumers_on_a_sparse_model():
    """predict(jacobians=True), linearize_predict_batch, one- and multi-step reachability and the resident server on a
    sparse model, against the existing oracle functions given the model's own beta and inv_K (project tolerances)."""
    from safe_exploration_amd import gp_reachability as reach, workload
    case = _headline()
    gp = _sparse_model(case)
    hyp, Zu = case["hyp"], case["Zu"]
    ls = np.stack([h["lengthscale"] for h in hyp])
    sf2 = np.array([h["variance"] for h in hyp])
    om = dict(Z=Zu, beta=gp.beta, inv_K=gp.inv_K, lengthscale=ls, signal_var=sf2)
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (40, 3))
    rmu, rvar, rjac = orc.gp_predict(x, Zu, om["beta"], om["inv_K"], ls, sf2, True)
    mu, var, jm, jv = gp.predict(x[:, :2], x[:, 2:], jacobians=True)
    outs = gp.linearize_predict_batch(x[:, :2], x[:, 2:])
    for got in ((mu, var, jm, jv), outs[:4]):
        np.testing.assert_allclose(got[0], rmu, rtol=1e-10, atol=mu_atol(om))
        np.testing.assert_allclose(got[1], rvar, rtol=0, atol=1e-9 * sf2.max())
        np.testing.assert_allclose(got[2], rjac, rtol=1e-10, atol=mu_atol(om) / ls.min())
    for t in (0, 17, 39):
        rjv, rhm = orc.gp_linearize_extras(x[t], Zu, om["beta"], om["inv_K"], ls, sf2)
        np.testing.assert_allclose(jv[t], rjv, rtol=1e-8, atol=1e-9 * sf2.max() / ls.min())
        np.testing.assert_allclose(outs[3][t], rjv, rtol=1e-8, atol=1e-9 * sf2.max() / ls.min())
        np.testing.assert_allclose(outs[4][t], rhm, rtol=1e-8, atol=100 * mu_atol(om))
    # reachability
    T = 33
    p = rng.uniform(-0.5, 0.5, (T, 2))
    k_ff = rng.uniform(-0.5, 0.5, (T, 1))
    k_fb = 0.1 * rng.standard_normal((T, 1, 2))
    q = np.stack([0.01 * (a.dot(a.T) + np.eye(2)) for a in rng.standard_normal((T, 2, 2))])
    l = np.array([0.05, 0.02])
    p1, q1, v1 = reach.onestep_reachability_batch(p, gp, k_ff, l, l, q, k_fb, 2.0, return_var=True)
    rp, rq, rv = orc.onestep_reachability_batch(om, p, q, k_ff, k_fb, l, l, 2.0)
    np.testing.assert_allclose(p1, rp, rtol=1e-10, atol=mu_atol(om))
    np.testing.assert_allclose(v1, rv, rtol=0, atol=1e-9 * sf2.max())
    np.testing.assert_allclose(q1, rq, rtol=1e-8, atol=1e-14)
    roll = workload.random_rollout_controls(12, 8, 3, 2, 1)
    a, b = 0.8 * np.eye(2), np.zeros((2, 1))
    pa, qa = reach.multistep_reachability_batch(roll["p0"], gp, roll["k_fb"], roll["k_ff"], l, l, None, 2.0, a, b)
    rpa, rqa = orc.multistep_reachability_batch(om, roll["p0"], roll["k_fb"], roll["k_ff"], l, l, None, 2.0, a, b)
    np.testing.assert_allclose(pa, rpa, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(qa, rqa, rtol=1e-7, atol=1e-13)
    # resident server: __call__ of one query
    gp.start_server()
    try:
        for t in (1, 5):
            m1, s1, j1 = gp(x[t:t + 1, :2], x[t:t + 1, 2:])
            np.testing.assert_allclose(np.ravel(m1), rmu[t], rtol=1e-10, atol=mu_atol(om))
            np.testing.assert_allclose(np.ravel(s1), rvar[t], rtol=0, atol=1e-9 * sf2.max())
            np.testing.assert_allclose(np.reshape(j1, (2, 3)), rjac[t], rtol=1e-10, atol=mu_atol(om) / ls.min())
        assert gp.server_state()[3] >= 2
    finally:
        gp.stop_server()


def test_refits_are_bit_identical_and_update_model_refits():
    case = R.make_case(9, "rbf", 2, 3, 96, 9001)
    states = []
    for _ in range(2):
        gp = _sparse_model(case, chunk=2048)
        a, w = gp.export_state()
        states.append((a.cpu().numpy(), w.cpu().numpy()))
    assert np.array_equal(states[0][0], states[1][0]) and np.array_equal(states[0][1], states[1][1])
    assert np.isfinite(states[0][1]).all() and np.array_equal(np.tril(states[0][1][0], -1), np.zeros_like(states[0][1][0]))
    # another chunk size: equal to rounding (the header promises bit-identity for one chunk size only)
    other = _sparse_model(case, chunk=512)
    np.testing.assert_allclose(other.predict(case["xq"])[1], gp.predict(case["xq"])[1], rtol=0, atol=1e-9)
    # update_model on a fixed-Z sparse model == train over the grown data
    from safe_exploration_amd import SimpleGPModel
    n0 = 6000
    g1 = SimpleGPModel(2, 2, 1, kern_types=case["kern_types"], hyp=case["hyp"], m=96, Z=case["Zu"])
    g1.do_sparse_gp = True
    g1.set_sparse_chunk(2048)
    g1.train(case["X"][:n0], case["Y"][:n0], 96, opt_hyp=False, Z=case["Zu"])
    g1.update_model(case["X"][n0:], case["Y"][n0:], replace_old=False)
    assert g1.x_train.shape[0] == 9001 and g1.is_sparse
    a1, w1 = g1.export_state()
    assert np.array_equal(a1.cpu().numpy(), states[0][0]) and np.array_equal(w1.cpu().numpy(), states[0][1])


def test_breakdown_is_reported_and_the_handle_stays_usable():
    from safe_exploration_amd import _lib, _buffers as B
    from safe_exploration_amd.ssm_hip import gaussian_process as G
    case = _headline()
    gp = _sparse_model(case)
    hd = gp._handle
    Zbad = case["Zu"].copy()
    Zbad[40] = Zbad[7]                                     # two identical inducing rows, no jitter: K_uu is singular
    s = B.stream_ptr(hd.device)
    gp._set_data(hd, Zbad, np.zeros((96, 2)), case["s2"], hd.device, s)
    tx, ty = B.as_dev(case["X"], hd.device), B.as_dev(case["Y"], hd.device)
    info = (ctypes.c_int * 2)()
    rc = _lib.lib.sr_gp_fit_sparse(hd.h, B.ptr(tx), B.ptr(ty), 3000, 0.0, s, info)
    # (which of the outputs -- both hold the two rows -- breaks down first is a matter of rounding: info names it)
    bad = [d for d in range(2) if info[d] != 0]
    assert rc == _lib.SR_ENOTPD and bad and all(1 <= info[d] <= 96 for d in bad), (rc, list(info), _lib.last_error())
    assert "output %d" % bad[0] in _lib.last_error() and "pivot %d" % info[bad[0]] in _lib.last_error()
    assert _lib.lib.sr_gp_is_sparse(hd.h) == 0
    with pytest.raises(np.linalg.LinAlgError):
        gp._train_sparse(case["X"], case["Y"], 96, False, 1e-5, Zbad, True, jitter=0.0)
    # bad arguments
    assert _lib.lib.sr_gp_fit_sparse(hd.h, B.ptr(tx), B.ptr(ty), 95, JIT, s, info) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_fit_sparse(hd.h, B.ptr(tx), B.ptr(ty), 3000, -1.0, s, info) == _lib.SR_EINVAL
    assert _lib.lib.sr_gp_fit_sparse(hd.h, None, B.ptr(ty), 3000, JIT, s, info) == _lib.SR_EINVAL
    # a good fit afterwards, on the same model
    ref = _sparse_model(case)
    gp.train(case["X"], case["Y"], 96, opt_hyp=False, Z=case["Zu"])
    assert np.array_equal(gp.predict(case["xq"])[1], ref.predict(case["xq"])[1])
    assert G.SPARSE_JITTER == 1e-6


def test_guarded_entries_on_a_sparse_handle():
    from safe_exploration_amd import _lib, _buffers as B
    case = _headline()
    gp = _sparse_model(case)
    hd = gp._handle
    lib, s = _lib.lib, B.stream_ptr(hd.device)
    out = B.empty((2,), hd.device)
    grad = B.empty((2, 3 + 3 * 3), hd.device)
    xn, yn = B.as_dev(case["X"][:1], hd.device), B.as_dev(case["Y"][:1], hd.device)
    info = (ctypes.c_int * 2)()
    host = (ctypes.c_double * 2)()
    x1, y1 = np.ascontiguousarray(case["X"][0]), np.ascontiguousarray(case["Y"][0])

    def guarded():
        return [lib.sr_gp_append(hd.h, B.ptr(xn), B.ptr(yn), 1, s, info),
                lib.sr_gp_append1_host(hd.h, ctypes.c_void_p(x1.ctypes.data), ctypes.c_void_p(y1.ctypes.data), s, info),
                lib.sr_gp_mll(hd.h, B.ptr(out), B.ptr(grad), s), lib.sr_gp_logdet(hd.h, B.ptr(out), s),
                lib.sr_gp_logdet_cached(hd.h, host)]
    assert lib.sr_gp_is_sparse(hd.h) == 1
    assert guarded() == [_lib.SR_ESTATE] * 5
    assert "sparse" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        gp.information_gain()
    assert lib.sr_gp_dims(hd.h, None, None, None, None) == 0
    # an exact fit on the inducing rows clears the mark
    assert lib.sr_gp_factorize(hd.h, s, info) == 0 and lib.sr_gp_is_sparse(hd.h) == 0
    assert lib.sr_gp_logdet(hd.h, B.ptr(out), s) == 0
    assert lib.sr_gp_append(hd.h, B.ptr(xn), B.ptr(yn), 1, s, info) == 0
    torch.cuda.synchronize()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _replica_worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from safe_exploration_amd import parallel
        case = _headline()
        gp = _sparse_model(case) if rank == 0 else None
        gp = parallel.replicate_model(gp, None, src=0)
        mu, var = gp.predict(case["xq"])
        ret[rank] = (mu.copy(), var.copy())
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_replicated_sparse_model_predicts_bit_identically(lib_built):
    import torch.multiprocessing as mp
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_replica_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
        assert np.array_equal(ret[0][0], ret[1][0]) and np.array_equal(ret[0][1], ret[1][1])
