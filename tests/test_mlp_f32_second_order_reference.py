"""CPU proof of the second-order reference of the fp32 network engine (tests/mlp_f32_second_order_reference.py).

Truth: the float64 passes are held to torch.float64 autograd double backward (create_graph=True) of the same MLP, an
independent derivation, to rtol 1e-10 (both are float64 and differ in summation order only). psi = act'' in the forward
value is held to central differences of the float64 phi; L_psi = sup |d psi / d y| to a dense grid. Tightness: a numpy
float32 emulation of the kernels' passes stays inside the per-element bounds, and the bounds are not vacuous: their median
over the abs-mode magnitude of the same quantity stays below a figure counted from the operations (test_bounds_...)."""
import numpy as np
import pytest
import torch

import mlp_f32_reference as F
import mlp_f32_second_order_reference as S
import mlp_reference as R

SMOOTH = ["Exponential", "Sigmoid", "Squareplus", "Softplus", "Tanh"]


def _torch_act(name, z):
    k = name.lower()
    if k == "none":
        return z
    if k == "relu":
        return torch.relu(z)
    if k == "leakyrelu":
        return torch.nn.functional.leaky_relu(z, 0.01)
    if k == "exponential":
        return torch.exp(z)
    if k == "sigmoid":
        return torch.sigmoid(z)
    if k == "squareplus":
        t = z * R.K_ACT
        return 0.5 * (t + torch.sqrt(t * t + 4.0)) / R.K_ACT
    if k == "softplus":
        return torch.nn.functional.softplus(z, beta=R.K_ACT, threshold=1e9)
    return torch.tanh(z)


def _autograd(mats, act, out_act, rows, dout, u0):
    """dL2/d(dout), dL2/dW_j, dL2/d(rows) of L2 = <u0, dL/d(rows)>, L = <dout, y>, by torch.float64 double backward"""
    Ws = [torch.tensor(m, dtype=torch.float64, requires_grad=True) for m in mats]
    e = torch.tensor(rows, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(dout, dtype=torch.float64, requires_grad=True)
    hcur = e
    for k, Wm in enumerate(Ws):
        hcur = _torch_act(act if k < len(Ws) - 1 else out_act, hcur @ Wm.T)
    de = torch.autograd.grad((hcur * g).sum(), e, create_graph=True)[0]
    L2 = (de * torch.tensor(u0, dtype=torch.float64)).sum()
    grads = torch.autograd.grad(L2, [g, e] + Ws, allow_unused=True)
    z = [np.zeros(t.shape) if gr is None else gr.numpy() for t, gr in zip([g, e] + Ws, grads)]
    return de.detach().numpy(), z[0], z[1], z[2:]


TRUTH_CASES = [(a, "None", NH) for a in R.ACTIVATIONS for NH in (0, 1, 2)] + [("ReLU", "Sigmoid", 2), ("Tanh", "Exponential", 1),
                                                                              ("None", "Softplus", 0), ("Squareplus", "Tanh", 2)]


@pytest.mark.parametrize("act,out_act,NH", TRUTH_CASES, ids=["%s-%s-h%d" % c for c in TRUTH_CASES])
def test_float64_passes_match_autograd_double_backward(act, out_act, NH):
    W, IN, OUTP, B = 16, 16, 16, 64
    rng = np.random.default_rng(11)
    if NH == 0:
        out_act = act if out_act == "None" else out_act  # a single matrix: the activation under test is the output's
    n = sum(r * c for r, c in F.shapes(W, IN, NH, OUTP))
    p = (rng.uniform(-1, 1, n) * 0.4).astype(np.float32)
    rows = rng.uniform(-1, 1, (B, IN)).astype(np.float32)
    dout = rng.uniform(-1, 1, (B, OUTP)).astype(np.float32)
    u0 = rng.uniform(-1, 1, (B, IN)).astype(np.float32)
    ref = S.reference(W, IN, NH, OUTP, act, out_act, p, rows, dout, u0)
    d0, ddout, de, dWs = _autograd(ref["mats"], act, out_act, rows, dout, u0)
    tol = dict(rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(ref["d0"], d0, **tol)
    np.testing.assert_allclose(ref["ddout"], ddout, **tol)
    np.testing.assert_allclose(ref["p0"], de, **tol)
    for a, b in zip(ref["wgrad"], dWs):
        np.testing.assert_allclose(a, b, **tol)
    if S.has_curvature(act) or S.has_curvature(out_act):
        assert np.abs(ref["p0"]).max() > 0
    else:
        assert ref["top"] == -1 and not ref["p0"].any()


@pytest.mark.parametrize("name", SMOOTH)
def test_psi_is_the_derivative_of_phi(name):
    """psi(y) = d phi / d z at y = act(z): central differences of the float64 phi(act(z)) in z"""
    lo, hi = (-3.0, 3.0) if name != "Exponential" else (-3.0, 5.0)
    z = np.linspace(lo, hi, 4001)
    hstep = 1e-5
    fd = (R.act_factor(name, R.act_forward(name, z + hstep)) - R.act_factor(name, R.act_forward(name, z - hstep))) / (2 * hstep)
    want = S.psi(name, R.act_forward(name, z))
    np.testing.assert_allclose(want, fd, rtol=1e-6, atol=1e-7 * max(1.0, np.abs(want).max()))
    for flat in ("None", "ReLU", "LeakyReLU"):
        assert not S.psi(flat, z).any() and not S.has_curvature(flat)


@pytest.mark.parametrize("name", SMOOTH)
def test_l_psi_on_a_dense_grid(name):
    """L_PSI bounds |d psi / d y| over the activation's range of forward values and is attained to 1 %; d psi / d y
    itself is held to central differences of psi"""
    k = name.lower()
    y = {"exponential": np.linspace(0.0, 50.0, 200001), "sigmoid": np.linspace(0.0, 1.0, 200001), "tanh": np.linspace(-1.0, 1.0, 200001),
         "softplus": np.linspace(0.0, 8.0, 800001), "squareplus": np.linspace(0.0, 8.0, 800001)}[k]
    d = S.dpsi_dy(name, y)
    hstep = 1e-6
    fd = (S.psi(name, y + hstep) - S.psi(name, y - hstep)) / (2 * hstep)
    np.testing.assert_allclose(d, fd, rtol=1e-5, atol=1e-5 * np.abs(d).max())
    assert np.abs(d).max() <= S.L_PSI[k] * (1 + 1e-12)
    assert np.abs(d).max() >= 0.99 * S.L_PSI[k]
    assert np.all(S.psi_abs_sum(name, y) >= np.abs(S.psi(name, y)) * (1 - 1e-12))


WORST = {}


def _mags(ref, NH):
    """the abs-mode magnitudes of dL2/d(dL/dy) and of the weight gradients: the same passes on absolute values"""
    A = [np.abs(m) for m in ref["mats"]]
    phi = [np.abs(np.asarray(ref["s"][j]) / np.where(ref["D"][j + 1] == 0, 1.0, ref["D"][j + 1])) for j in range(NH + 1)]
    mD = [None] * (NH + 2)
    mD[NH + 1] = np.abs(ref["D"][NH + 1])
    ms = [None] * (NH + 1)
    for j in range(NH, -1, -1):
        ms[j] = mD[j + 1] * phi[j]
        mD[j] = ms[j] @ A[j]
    mU, mR = [np.abs(ref["Uc"][0])], [None] * (NH + 1)
    for j in range(NH + 1):
        mT = mU[j] @ A[j].T
        mU.append(mT * phi[j])
        if ref["Rr"][j] is not None:
            mR[j] = mT * mD[j + 1] * np.abs(ref["Rr"][j] / np.where(ref["T"][j] * ref["D"][j + 1] == 0, 1.0, ref["T"][j] * ref["D"][j + 1]))
    mQ = [None] * (NH + 1)
    for j in range(ref["top"], -1, -1):
        if j == ref["top"]:
            mQ[j] = mR[j]
        if j > 0:
            mQ[j - 1] = (mQ[j] @ A[j]) * phi[j - 1] + (mR[j - 1] if mR[j - 1] is not None else 0.0)
    mw = [ms[j].T @ mU[j] + (mQ[j].T @ np.abs(ref["h"][j]) if mQ[j] is not None else 0.0) for j in range(NH + 1)]
    return mU[NH + 1], mw


def vacuity_figure(case, B):
    """A rounding made at one of n sites reaches a result once directly -- through |W| and |phi|, which the abs-mode
    magnitude already carries -- and once through every factor phi_j or psi_j evaluated from a forward value it has moved,
    amplified there by L_phi or L_psi: at most 1 + sum over the layers of (L_phi + L_psi). The sites on a path: the four
    chains per layer (forward, first-order backward, tangent, curvature: 4 sum K_j terms), one slab chain and its
    2 n_slabs additions, and at most 30 formula roundings per layer (phi, psi, the products, the measured library
    accuracies in units of u). figure = u * sites * amplification."""
    names = [case.act] * case.NH + [case.out_act]
    Ks = [c for _, c in F.shapes(case.W, case.IN, case.NH, case.OUTP)]
    sites = 4 * sum(Ks) + F.SLAB_ROWS + 2 * (B // F.SLAB_ROWS) + 30 * (case.NH + 1)
    amp = 1.0 + sum(F.L_PHI.get(n.lower(), 0.0) + S.L_PSI.get(n.lower(), 0.0) for n in names)
    return S.U * sites * amp


@pytest.mark.parametrize("B", S.BATCHES)
@pytest.mark.parametrize("case", S.CASES, ids=[c.id for c in S.CASES])
def test_float32_emulation_is_within_the_bounds_which_are_not_vacuous(case, B):
    x, rows, dout, u_x, p, ref = S.setup_identity(case, B)
    u0 = S.identity_u0(u_x, case.IN).astype(np.float32)
    ddout, wg, p0 = S.eval_f32(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, dout, u0)
    ratios = S.check(ref, ddout, wg, case.NH, case.id)
    want_dx, e_dx = S.identity_dinput(ref, case.n_in)
    ratios["dinput"] = S.check_one("dinput", p0[:, :case.n_in], want_dx, e_dx, case.id)
    WORST[(case.id, B)] = ratios
    print(case.id, B, ratios)
    # not vacuous
    fig = vacuity_figure(case, B)
    m_dd, m_w = _mags(ref, case.NH)
    # (the padded outputs have zero weights and zero dL/dy: no magnitude, and nothing but the floor as a bound)
    meds = {"ddout": float(np.median((ref["e_ddout"] / np.where(m_dd == 0, 1.0, m_dd))[:, :case.n_out]))}
    for name, ew, mw in zip(R.matrix_names(case.NH), ref["e_w"], m_w):
        # likewise the rows of the padded outputs, and the first matrix's columns of the padding inputs (U_0 is zero there:
        # term A has no magnitude)
        rws = slice(0, case.n_out) if name == "Wout" else slice(None)
        cls = slice(0, case.n_in) if name in ("W0",) or case.NH == 0 else slice(None)
        meds[name] = float(np.median(ew[rws, cls] / mw[rws, cls]))
    print(case.id, B, "median bound / abs-mode magnitude", meds, "figure", fig)
    for k, v in meds.items():
        assert v <= fig, (case.id, k, v, fig)


def test_a_moved_element_fails():
    """one element of dL2/d(dL/dy) and one of the first matrix's gradient moved by 2^-10 of its abs-mode magnitude"""
    case = next(c for c in S.CASES if c.name == "w16h1" and c.act == "Softplus")
    x, rows, dout, u_x, p, ref = S.setup_identity(case, 256)
    u0 = S.identity_u0(u_x, case.IN).astype(np.float32)
    ddout, wg, p0 = S.eval_f32(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, dout, u0)
    m_dd, m_w = _mags(ref, case.NH)
    bad = ddout.copy()
    j = int(np.argmax(m_dd))
    bad.flat[j] += np.float32(2.0 ** -10 * m_dd.flat[j])
    with pytest.raises(AssertionError):
        S.check(ref, bad, wg, case.NH)
    badw = wg.copy()
    j = int(np.argmax(m_w[0]))
    badw[j] += np.float32(2.0 ** -10 * m_w[0].flat[j])
    with pytest.raises(AssertionError):
        S.check(ref, ddout, badw, case.NH)


def test_branch_filter_keeps_half_of_the_candidates():
    """ReLU / LeakyReLU rows: the float64 reference alone keeps at least B of the 2 B candidates at both batch sizes"""
    for case in S.CASES:
        if case.act.lower() in F.BRANCHY:
            for B in S.BATCHES:
                x2, _, _ = S.case_inputs(case, B)
                ok = F.clear_of_branches(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, F.case_params(case), F.identity_rows(case, x2))
                assert ok.sum() >= B, (case.id, B, int(ok.sum()))
