"""Second-order input gradients of the fp32 network engine (NetworkF32Host::backward_backward_input, csrc/mlp_f32.hip)
against float64: the exact passes, the curvature factors psi = act'' in the stored forward value, per-element bounds
that extend rules (1)-(6) of tests/mlp_f32_reference.py, and a numpy float32 emulation of the kernels' arithmetic.
Plain numpy; shared by tests/test_mlp_f32_second_order_reference.py (CPU) and the GPU tests.

Notation (per batch row). Layer j = 0..NH maps h_j to h_{j+1} = a_j(W_j h_j); h_0 = e is the encoded row, y = h_{NH+1}.
First order: D_{NH+1} = dL/dy, s_j = D_{j+1} o phi_j(h_{j+1}), dW_j = sum_b s_j h_j^T, D_j = s_j W_j. Second order, from
U_0 = dL2/dD_0 (the encoding's step; Identity: scale * u_x in the value columns, 0 in the padding):

  tangent    T_j = U_j W_j^T,  U_{j+1} = T_j o phi_j(h_{j+1}),  term A: dL2/dW_j += sum_b s_j U_j^T;  U_{NH+1} = dL2/d(dL/dy)
  curvature  R_j = (T_j o D_{j+1}) o psi_j(h_{j+1});  Q_NH = R_NH,  P_j = Q_j W_j,  term B: dL2/dW_j += sum_b Q_j h_j^T,
             Q_{j-1} = R_{j-1} + P_j o phi_{j-1}(h_j);  P_0 = dL2/de goes through the encoding's first-order backward.

Bounds (u = 2^-24; no figure comes from the kernels). Rules (1)-(6) of mlp_f32_reference.py hold as they stand: the
forward errors e_h and the first-order transfer s_j with its bound e_s are computed exactly as there. New here:

  (7) a tangent value is an operand with its own bound: T_j is chain (1) over K_j terms with operand error e_U,
      e_T = e_U |W|^T + K u (|U| + e_U) |W|^T; U_{j+1} = T phi is the product of rule (3),
      e = e_T |phi| + (|T| + e_T) e_phi + u (|T| + e_T)(|phi| + e_phi) (None copies T; ReLU keeps or drops it; LeakyReLU
      is one multiplication by an exact factor). The Identity step is one multiplication: e_U0 = u |U_0|.
  (8) psi is computed from the computed y: e_psi = L_psi e_y + n u M, n the roundings of the formula in csrc/act_f32.h
      (act_factor2_f32, evaluated as written: the library is built with contraction off) and M the abs-sum of its terms:
        Exponential  psi = y                         n = 0                 L_psi = 1
        Sigmoid      (y (1 - y)) (1 - 2 y)            n = 4, M = |y| (1 + |y|)(1 + 2 |y|)   L_psi = 1   (|1 - 6 y + 6 y^2| on [0, 1])
        Tanh         (-2 y)(1 - y y)                  n = 3, M = 2 |y| (1 + y^2)            L_psi = 4   (|-2 + 6 y^2| on [-1, 1])
        Softplus     K ((1 - E) E), E = expf(-y K)    n = 3, M = K (1 + E) E                L_psi = K^2 = 100  (K^2 E |1 - 2 E|, E -> 1)
        Squareplus   2K t^3 / (t^2 + 1)^3, t = y K    n = 21, M = |psi|                     L_psi = 46.5
      Squareplus: every term is positive, so relative errors add: t 1, t^2 3, d = t^2 + 1 4, t^3 5, 2K t^3 6, d^2 9, d^3 14,
      the quotient 6 + 14 + 1 = 21. Its L_psi = 6 K^2 max s |1 - s| / (1 + s)^4 (s = t^2) = 600 * 0.07746 at s = (5 - sqrt 17) / 4.
      Softplus's E carries the expf accuracy profiles/act_f32_ulps.json records for its factor 1 - E: |E_c - E| <=
      e_E = (2 c_factor + 1) u (the measured error of 1 - E, doubled off the grid, plus the subtraction's own rounding;
      0 <= 1 - E < 1), which enters psi through d/dE (1 - E) E = 1 - 2 E, |.| <= 1: + K (e_E + e_E^2). Exponential adds
      its recorded factor accuracy 2 c_factor u max(|y|, 1) in the same way (the record is 0: psi = y has no formula).
      L_psi is verified on a dense grid by the CPU test.
      R = (T D) psi is two products of rule (3): first T D with (e_T, e_D), then with (e_psi).
  (9) the curvature chain: P_j is rule (4) with operand error e_Q; Q_{j-1} = P phi (+ R) is rule (3)'s product and one
      addition: + u (|P phi| + e + |R| + e_R).
  (10) a matrix's gradient is term A (operands s_j with e_s, U_j with e_U) plus term B (Q_j with e_Q, h_j with e_h),
      each in slabs of SLAB_ROWS rows summed in one fixed-order sum of 2 n_slabs slab values (n_slabs without term B):
      rule (5) with (SLAB_ROWS + 2 n_slabs) u over the two magnitudes together.
"""
import numpy as np

import mlp_f32_reference as F
import mlp_reference as R

U = F.U
K = R.K_ACT
FLOOR = F.FLOOR
SMOOTH = ("exponential", "sigmoid", "tanh", "softplus", "squareplus")
L_PSI = {"exponential": 1.0, "sigmoid": 1.0, "tanh": 4.0, "softplus": K * K, "squareplus": 46.5}
PSI_ROUNDINGS = {"exponential": 0, "sigmoid": 4, "tanh": 3, "softplus": 3, "squareplus": 21}


def has_curvature(name):
    return name.lower() in SMOOTH


def psi(name, y):
    """d^2 act / d z^2 written in the forward value y (float64)"""
    k = name.lower()
    if k == "exponential":
        return y
    if k == "sigmoid":
        return y * (1.0 - y) * (1.0 - 2.0 * y)
    if k == "tanh":
        return -2.0 * y * (1.0 - y * y)
    if k == "softplus":
        E = np.exp(-K * y)
        return K * (1.0 - E) * E
    if k == "squareplus":
        t = K * y
        return 2.0 * K * t ** 3 / (t * t + 1.0) ** 3
    return np.zeros_like(y)


def dpsi_dy(name, y):
    """d psi / d y (float64): what L_PSI bounds"""
    k = name.lower()
    if k == "exponential":
        return np.ones_like(y)
    if k == "sigmoid":
        return 1.0 - 6.0 * y + 6.0 * y * y
    if k == "tanh":
        return -2.0 + 6.0 * y * y
    if k == "softplus":
        E = np.exp(-K * y)
        return -K * K * E * (1.0 - 2.0 * E)
    t = K * y
    return 6.0 * K * K * t * t * (1.0 - t * t) / (t * t + 1.0) ** 4


def psi_abs_sum(name, y):
    k = name.lower()
    a = np.abs(y)
    if k == "sigmoid":
        return a * (1.0 + a) * (1.0 + 2.0 * a)
    if k == "tanh":
        return 2.0 * a * (1.0 + a * a)
    if k == "softplus":
        E = np.exp(-K * y)
        return K * (1.0 + E) * E
    return np.abs(psi(name, y))


def psi_error(name, y, ey):
    """rule (8)"""
    k = name.lower()
    e = L_PSI[k] * ey + PSI_ROUNDINGS[k] * U * psi_abs_sum(name, y)
    c = F.ULPS[F._NAMES[k]]["factor"]
    if k == "softplus":
        eE = (2.0 * c + 1.0) * U
        e = e + K * (eE + eE * eE)
    elif k == "exponential":
        e = e + 2.0 * c * U * np.maximum(np.abs(y), 1.0)
    return e


def _product(a, ea, b, eb):
    """rule (3): the bound of the rounded product of two computed values"""
    return ea * np.abs(b) + (np.abs(a) + ea) * eb + U * (np.abs(a) + ea) * (np.abs(b) + eb)


def _phi(name, y, ey):
    """(phi, e_phi) of the transfer factor from the stored forward value, rule (3); exact for None / ReLU / LeakyReLU"""
    kk = name.lower()
    phi = R.act_factor(name, y)
    if kk in ("none",) + F.BRANCHY:
        return phi, np.zeros_like(phi)
    return phi, F.L_PHI[kk] * ey + 2 * F._act_terms(name)[1] * U * np.maximum(np.abs(phi), 1.0)


def _gate(name, t, et, y, ey):
    """(t o phi, its bound): the engine's bwd_act on a computed t"""
    kk = name.lower()
    phi, ephi = _phi(name, y, ey)
    if kk == "none":
        return t, et
    if kk == "relu":
        return t * phi, et * phi
    if kk == "leakyrelu":
        return t * phi, et * phi + U * np.abs(t * phi)
    return t * phi, _product(t, et, phi, ephi)


def identity_u0(u_x, IN, scale=1.0):
    u_x = np.asarray(u_x, np.float64)
    u0 = np.zeros((u_x.shape[0], IN))
    u0[:, :u_x.shape[1]] = scale * u_x
    return u0


def reference(W, IN, NH, OUTP, act, out_act, params, rows, dout, u0, e_u0=None, e_d0_extra=None):
    """float64 truth and bounds of the second-order passes for fp32 parameters params [n_mlp], encoded rows [B][IN]
    (taken as exact), dL/dy dout [B][OUTP] and U_0 = u0 [B][IN] with its own bound e_u0 (None: rule (7)'s Identity step).
    Returns a dict: ddout [B][OUTP] (U_{NH+1}), wgrad [per matrix], p0 [B][IN] (dL2/de; zeros without curvature), d0
    [B][IN] (the first-order D_0) and the bounds e_ddout, e_w, e_p0, e_d0; plus the chains D, Uc, T, Rr, Q for the tests."""
    first = F.reference(W, IN, NH, OUTP, act, out_act, params, rows, dout)
    mats = [m.astype(np.float64) for m in F.split(W, IN, NH, OUTP, np.asarray(params))]
    rows, dout, u0 = (np.asarray(v, np.float64) for v in (rows, dout, u0))
    B = rows.shape[0]
    names = [act] * NH + [out_act]
    h = [rows] + first["hidden"] + [first["out"]]
    eh = [np.zeros_like(rows)] + list(first["e_hidden"]) + [first["e_out"]]
    n_slabs = (B + F.SLAB_ROWS - 1) // F.SLAB_ROWS

    # the first-order chain, every delta kept: D[j] = dL/dh_j, s[j] = D[j+1] o phi_j
    D, eD = [None] * (NH + 2), [None] * (NH + 2)
    s, es = [None] * (NH + 1), [None] * (NH + 1)
    D[NH + 1], eD[NH + 1] = dout, np.zeros_like(dout)
    for j in range(NH, -1, -1):
        s[j], es[j] = _gate(names[j], D[j + 1], eD[j + 1], h[j + 1], eh[j + 1])
        A = np.abs(mats[j])
        D[j] = s[j] @ mats[j]
        eD[j] = es[j] @ A + mats[j].shape[0] * U * ((np.abs(s[j]) + es[j]) @ A) + FLOOR
    assert np.allclose(D[0], first["dinput"], rtol=1e-12, atol=1e-300)

    # tangent pass
    Uc, eU = [None] * (NH + 2), [None] * (NH + 2)
    T, eT = [None] * (NH + 1), [None] * (NH + 1)
    Rr, eR = [None] * (NH + 1), [None] * (NH + 1)
    Uc[0] = u0
    eU[0] = U * np.abs(u0) if e_u0 is None else np.asarray(e_u0, np.float64)
    for j in range(NH + 1):
        A = np.abs(mats[j]).T
        T[j] = Uc[j] @ mats[j].T
        eT[j] = eU[j] @ A + mats[j].shape[1] * U * ((np.abs(Uc[j]) + eU[j]) @ A) + FLOOR
        Uc[j + 1], eU[j + 1] = _gate(names[j], T[j], eT[j], h[j + 1], eh[j + 1])
        if has_curvature(names[j]):
            td, etd = T[j] * D[j + 1], _product(T[j], eT[j], D[j + 1], eD[j + 1])
            ps = psi(names[j], h[j + 1])
            Rr[j], eR[j] = td * ps, _product(td, etd, ps, psi_error(names[j], h[j + 1], eh[j + 1]))

    # curvature pass
    top = max([j for j in range(NH + 1) if Rr[j] is not None], default=-1)
    Q, eQ = [None] * (NH + 1), [None] * (NH + 1)
    p0, e_p0 = np.zeros_like(rows), np.zeros_like(rows)
    for j in range(top, -1, -1):
        if j == top:
            Q[j], eQ[j] = Rr[j], eR[j]
        A = np.abs(mats[j])
        P = Q[j] @ mats[j]
        eP = eQ[j] @ A + mats[j].shape[0] * U * ((np.abs(Q[j]) + eQ[j]) @ A) + FLOOR
        if j == 0:
            p0, e_p0 = P, eP
            break
        g, eg = _gate(names[j - 1], P, eP, h[j], eh[j])
        if Rr[j - 1] is not None:
            Q[j - 1] = g + Rr[j - 1]
            eQ[j - 1] = eg + eR[j - 1] + U * (np.abs(g) + eg + np.abs(Rr[j - 1]) + eR[j - 1])
        else:
            Q[j - 1], eQ[j - 1] = g, eg

    # the weight gradients: term A + term B in one sum
    wgrad, e_w = [None] * (NH + 1), [None] * (NH + 1)
    for j in range(NH + 1):
        ds, aU = np.abs(s[j]) + es[j], np.abs(Uc[j]) + eU[j]
        wgrad[j] = s[j].T @ Uc[j]
        e = es[j].T @ aU + np.abs(s[j]).T @ eU[j]
        mag = ds.T @ aU
        parts = n_slabs
        if Q[j] is not None:
            dq, ah = np.abs(Q[j]) + eQ[j], np.abs(h[j]) + eh[j]
            wgrad[j] = wgrad[j] + Q[j].T @ h[j]
            e = e + eQ[j].T @ ah + np.abs(Q[j]).T @ eh[j]
            mag = mag + dq.T @ ah
            parts = 2 * n_slabs
        e_w[j] = e + (F.SLAB_ROWS + parts) * U * mag + FLOOR
    return dict(ddout=Uc[NH + 1], e_ddout=eU[NH + 1], wgrad=wgrad, e_w=e_w, p0=p0, e_p0=e_p0, d0=D[0], e_d0=eD[0], top=top,
                D=D, Uc=Uc, T=T, Rr=Rr, Q=Q, s=s, h=h, mats=mats, mag_w=[np.abs(a).T @ np.abs(b) for a, b in zip(s, Uc[:-1])])


def identity_dinput(ref, n_in, scale=1.0):
    """(dL2/dinput, bound) behind Identity: P_0's value columns times the scale (one multiplication)"""
    v = ref["p0"][:, :n_in] * scale
    return v, ref["e_p0"][:, :n_in] * abs(scale) + U * np.abs(v) + FLOOR


def check(ref, ddout, wgrad_flat, NH, label=""):
    """every element of dL2/d(dL/dy) and of every matrix's gradient within its bound; returns the worst ratios"""
    ratios = {}

    def one(name, got, want, bound):
        q = np.abs(np.asarray(got, np.float64) - want) / bound
        q = np.where(np.isnan(q), np.inf, q)
        j = int(np.argmax(q))
        ratios[name] = float(q.flat[j])
        assert q.flat[j] <= 1.0, (label, name, float(q.flat[j]), j, float(np.asarray(got).flat[j]), float(want.flat[j]))

    if ddout is not None:
        one("ddout", ddout, ref["ddout"], ref["e_ddout"])
    if wgrad_flat is not None:
        off = 0
        for name, w, ew in zip(R.matrix_names(NH), ref["wgrad"], ref["e_w"]):
            one(name, np.asarray(wgrad_flat)[off:off + w.size].reshape(w.shape), w, ew)
            off += w.size
        assert off == np.asarray(wgrad_flat).size
    return ratios


def check_one(name, got, want, bound, label=""):
    q = np.abs(np.asarray(got, np.float64) - want) / bound
    q = np.where(np.isnan(q), np.inf, q)
    j = int(np.argmax(q))
    assert q.flat[j] <= 1.0, (label, name, float(q.flat[j]), j, float(np.asarray(got).flat[j]), float(np.asarray(want).flat[j]))
    return float(q.flat[j])


# ---- a numpy float32 evaluation: the arithmetic of the kernels ----
def _psi32(name, y):
    k, f = name.lower(), np.float32
    kk = f(K)
    if k == "exponential":
        return y
    if k == "sigmoid":
        return ((y * (f(1) - y)).astype(f) * (f(1) - f(2) * y)).astype(f)
    if k == "tanh":
        return ((f(-2) * y) * (f(1) - (y * y).astype(f))).astype(f)
    if k == "softplus":
        e = np.exp(-y * kk).astype(f)
        return (kk * ((f(1) - e) * e).astype(f)).astype(f)
    t = (y * kk).astype(f)
    t2 = (t * t).astype(f)
    d = (t2 + f(1)).astype(f)
    return ((f(2) * kk) * (t2 * t).astype(f) / ((d * d).astype(f) * d).astype(f)).astype(f)


def _slab_sum(parts):
    s = parts[0].astype(np.float32)
    for t in parts[1:]:
        s = (s + t).astype(np.float32)
    return s


def eval_f32(W, IN, NH, OUTP, act, out_act, params, rows, dout, u0):
    """(ddout, flat wgrad, p0) in float32 arithmetic, slab sums as the engine orders them"""
    f = np.float32
    mats = F.split(W, IN, NH, OUTP, np.asarray(params, f))
    names = [act] * NH + [out_act]
    _, hidden, _, _ = F.eval_f32(W, IN, NH, OUTP, act, out_act, params, rows, dout)
    h = [np.asarray(rows, f)] + list(hidden)
    h.append(F._act32(out_act, (h[NH] @ mats[NH].T).astype(f)).astype(f))
    B = h[0].shape[0]

    def gate(name, t, y):
        return t if name.lower() == "none" else (t * F._factor32(name, y)).astype(f)

    D = [None] * (NH + 2)
    D[NH + 1] = np.asarray(dout, f)
    for j in range(NH, -1, -1):
        D[j] = (gate(names[j], D[j + 1], h[j + 1]) @ mats[j]).astype(f)
    Uc, Rr = [np.asarray(u0, f)], [None] * (NH + 1)
    for j in range(NH + 1):
        T = (Uc[j] @ mats[j].T).astype(f)
        Uc.append(gate(names[j], T, h[j + 1]))
        if has_curvature(names[j]):
            Rr[j] = ((T * D[j + 1]).astype(f) * _psi32(names[j], h[j + 1])).astype(f)
    top = max([j for j in range(NH + 1) if Rr[j] is not None], default=-1)
    Q = [None] * (NH + 1)
    p0 = np.zeros((B, IN), f)
    for j in range(top, -1, -1):
        if j == top:
            Q[j] = Rr[j]
        P = (Q[j] @ mats[j]).astype(f)
        if j == 0:
            p0 = P
            break
        g = gate(names[j - 1], P, h[j])
        Q[j - 1] = (g + Rr[j - 1]).astype(f) if Rr[j - 1] is not None else g
    wg = []
    for j in range(NH + 1):
        sj = gate(names[j], D[j + 1], h[j + 1])
        sl = range(0, B, F.SLAB_ROWS)
        parts = [sj[b:b + F.SLAB_ROWS].T @ Uc[j][b:b + F.SLAB_ROWS] for b in sl]
        if Q[j] is not None:
            parts += [Q[j][b:b + F.SLAB_ROWS].T @ h[j][b:b + F.SLAB_ROWS] for b in sl]
        wg.append(_slab_sum(parts))
    return Uc[NH + 1], np.concatenate([w.ravel() for w in wg]), p0


# ---- the cases of the GPU test: the smallest shapes that reach every path ----
def _cases():
    C = F.Case
    c = []
    for a in R.ACTIVATIONS:  # every trainable activation: W 64 with IN 32 (two k steps, output padded to 16), NH 2
        s = 0.6 if a == "Exponential" else 1.0
        c.append(C("w64in32h2", 64, 2, n_in=19, n_out=3, act=a, scale=s, otype="FullyFusedMLP"))
    c.append(C("w16h1", 16, 1, n_in=3, n_out=1, act="Softplus", otype="FullyFusedMLP"))   # the two-accumulator path
    c.append(C("w16h1", 16, 1, n_in=3, n_out=1, act="ReLU", otype="FullyFusedMLP"))
    c.append(C("w144h1", 144, 1, n_in=16, n_out=3, act="Tanh", scale=1.0))                # 2 x 64 + 16: a partial column group
    c.append(C("h0", 64, 0, n_in=16, n_out=17, act="Sigmoid", out_act="Sigmoid"))         # one matrix, smooth output, OUTP 32
    c.append(C("w48h2", 48, 2, n_in=16, n_out=3, act="ReLU", out_act="Sigmoid"))          # curvature at the top only
    c.append(C("w48h2", 48, 2, n_in=16, n_out=3, act="Tanh", out_act="Exponential", scale=0.6))
    return c


CASES = _cases()
BATCHES = (256, 768)  # 256: two 128-row workgroups; 768: three weight-gradient slabs


def case_inputs(case, B, seed=0):
    """2 B candidate input rows (Identity: uniform [-1, 1]), dL/dy [B][OUTP] and u_x = dL2/d(dL/dx) [B][n_in], uniform [-1, 1]"""
    x, dout = F.case_inputs(case, B, seed)
    u_x = np.random.default_rng(2000 + seed).uniform(-1.0, 1.0, (B, case.n_in)).astype(np.float32)
    return x, dout, u_x


def setup_identity(case, B, seed=0):
    """(x [B][n_in], rows [B][IN], dout, u_x, params, second-order reference) of a Network alone; rows kept clear of
    the ReLU / LeakyReLU branches by the float64 reference alone (at least B of the 2 B candidates, else this fails)"""
    x2, dout, u_x = case_inputs(case, B, seed)
    p = F.case_params(case)
    x, rows = F.keep_clear(case, p, x2, F.identity_rows(case, x2), B)
    ref = reference(case.W, case.IN, case.NH, case.OUTP, case.act, case.out_act, p, rows, dout, identity_u0(u_x, case.IN))
    return x, rows, dout, u_x, p, ref
