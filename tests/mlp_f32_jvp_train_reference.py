"""dL/dparams of L = sum C_y o y + sum C_J o Jv for an fp32 FullyFusedMLP behind a lone grid or Identity
(csrc/mlp_f32_jvp_train.hip): the float64 truth and a per-element bound, for tests/test_gpu_mlp_f32_jvp_train.py.

Truth: torch.float64 on the CPU. The grid is sum_c w_c table[idx_c] with the entries of
test_grid_f32_reference.level_corners and weights (and their x-derivatives) recomputed in float64 from
test_gpu_mlp_f32_jvp.fractions; they do not depend on the parameters. t_0 = (de/dx) v, s_j = W_j t_j,
t_{j+1} = a_j'(z_j) s_j with plain torch operations, and dL/dparams from L.backward().

Bound: every computed quantity is carried as (value, error bound) through the kernels' operations in their order, by
rules (1)-(10) of mlp_f32_reference.py and mlp_f32_second_order_reference.py, whose functions do the work (u = 2^-24):
  rows      h_0 errs by test_grid_f32_reference.forward_bound, t_0 by test_gpu_mlp_f32_jvp.encoding_jacobian's bound
            plus D u sum |de/dx| |v| for the direction sum; behind an Identity both are one rounding.
  forward   mlp_f32_reference.reference gives e_h of every stored value from e_h0 (rules 1, 2); a tangent is rule (7):
            s_j a K_j-term chain with operand error, t_{j+1} = s_j phi the product of rule (3) with
            e_phi = L_PHI e_y + 2 c u max(|phi|, 1) per activation.
  reverse   sb_k and phi hb are rule (3)'s product again; the curvature term is sum_k s_k tb_k (K products and K
            additions), times psi with rule (8)'s e_psi = L_PSI e_y + roundings, added to phi hb (rule 9: one rounding).
            hb_j, tb_j are rule (4) over N_j terms.
  weights   rule (5) over the (1 + K) B stacked rows: e_G^T (|X| + e_X) + |G|^T e_X + (SLAB_ROWS + n_slabs) u mags.
  table     value term: test_grid_f32_reference.gradient_bound (int32 fixed point included) at |hb_0| + e_hb0, plus
            sum w e_hb0. Tangent term, per (point, corner): the coefficient dw_c/dx_d has 2 (D - 1) + 3 roundings
            (+ 3 and the absolute term 4 u scale pd S_d for Smoothstep, as encoding_jacobian argues), G_d = sum_k v tb_0
            is K terms, the sum over d D terms; the atomics add count_p terms in any order: count_p u sum |term|; the
            final add of the two parts is one rounding.
No figure comes from a GPU result.
"""
import numpy as np

import mlp_f32_reference as F
import mlp_f32_second_order_reference as S2
import test_gpu_mlp_f32_jvp as V
import test_grid_f32_reference as G

U = F.U


def corners(g, l, x):
    """level l: entries idx [B][NC], weights w, Smoothstep sensitivity S (level_corners), dw/dx [B][NC][D] and
    SD [B][NC][D] = scale pd_d sum_{e != d} s_e prod_{e' != d, e} a_e' (zero for Linear)"""
    assert g.interpolation != 0
    idx, w, S = G.level_corners(g, l, x)
    B, D = x.shape
    smooth, f, scale = g.interpolation == 2, V.fractions(g, l, x), float(np.float32(g.scales[l]))
    s = f * f * (3.0 - 2.0 * f) if smooth else f
    pd = 6.0 * f * (1.0 - f) if smooth else np.ones_like(f)
    dw, SD = np.zeros((B, 1 << D, D)), np.zeros((B, 1 << D, D))
    for c in range(1 << D):
        a = np.where([bool(c >> d & 1) for d in range(D)], s, 1.0 - s)
        for d in range(D):
            o = [e for e in range(D) if e != d]
            dw[:, c, d] = (1.0 if c >> d & 1 else -1.0) * scale * pd[:, d] * np.prod(a[:, o], axis=1)
            if smooth:
                SD[:, c, d] = scale * pd[:, d] * sum(s[:, e] * np.prod(a[:, [k for k in o if k != e]], axis=1) for e in o)
    return idx, w, S, dw, SD


def truth(torch, case, enc, g, p, x, v, Cy, CJ):
    """dL/dparams, float64 [n_params]; v [B][K][D]"""
    B, D = x.shape
    q = torch.from_numpy(p).double().requires_grad_(True)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    mats, off = [], 0
    for r, c in F.shapes(case.W, case.IN, case.NH, case.OUTP):
        mats.append(q[off:off + r * c].reshape(r, c))
        off += r * c
    h, t = torch.zeros(B, case.IN, dtype=torch.float64), torch.zeros(v.shape[1], B, case.IN, dtype=torch.float64)
    if g is None:
        s, o = float(np.float32(enc["scale"])), float(np.float32(enc["offset"]))
        h[:, D:] = 1.0
        h[:, :D] = t64(x) * s + o
        t[:, :, :D] = t64(v).permute(1, 0, 2) * s
    else:
        Fe, tab, hs, ts = g.n_features_per_level, q[off:].reshape(-1, g.n_features_per_level), [], []
        for l in range(g.n_levels):
            idx, w, _, dw, _ = corners(g, l, x)
            e = tab[torch.from_numpy(idx)]  # [B][NC][Fe]
            hs.append(torch.einsum("bc,bcf->bf", t64(w), e))
            ts.append(torch.einsum("bcd,bkd,bcf->kbf", t64(dw), t64(v), e))
        pad = case.IN - g.n_levels * Fe
        h = torch.cat(hs + [h[:, :pad]], 1)
        t = torch.cat(ts + [t[:, :, :pad]], 2)
    for j, M in enumerate(mats):
        name = (case.act if j < case.NH else case.out_act).lower()
        z, s = h @ M.T, t @ M.T
        h = {"none": lambda z: z, "relu": torch.relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid,
             "softplus": lambda z: torch.nn.functional.softplus(z * 10.0, threshold=1e9) / 10.0}[name](z)
        t = s if name == "none" else torch.autograd.grad(h.sum(), z, create_graph=True)[0] * s
    ((t64(Cy) * h).sum() + (t64(CJ) * t[:, :, :case.n_out].permute(1, 2, 0)).sum()).backward()
    return q.grad.numpy()


def encoded(case, enc, g, p, x, v):
    """h_0, e_h0 [B][IN] and t_0, e_t0 [K][B][IN], float64"""
    B, D = x.shape
    v64 = v.astype(np.float64)
    h0, e0 = np.zeros((B, case.IN)), np.zeros((B, case.IN))
    if g is None:
        s, o = float(np.float32(enc["scale"])), float(np.float32(enc["offset"]))
        h0[:, D:] = 1.0
        h0[:, :D] = x.astype(np.float64) * s + o
        e0[:, :D] = U * np.abs(h0[:, :D])
        t0 = np.zeros((v.shape[1], B, case.IN))
        t0[:, :, :D] = v64.transpose(1, 0, 2) * s
        return h0, e0, t0, U * np.abs(t0)
    Fe, tab = g.n_features_per_level, p[case.n_mlp:].astype(np.float64).reshape(-1, g.n_features_per_level)
    for l in range(g.n_levels):
        idx, w, S, _, _ = corners(g, l, x)
        e = tab[idx]
        h0[:, l * Fe:(l + 1) * Fe] = np.einsum("bc,bcf->bf", w, e)
        e0[:, l * Fe:(l + 1) * Fe] = G.forward_bound(g, np.einsum("bc,bcf->bf", w, np.abs(e)), np.einsum("bc,bcf->bf", S, np.abs(e)))
    dE, err = V.encoding_jacobian(g, x, p[case.n_mlp:], case.IN)
    t0 = np.einsum("bcd,bkd->kbc", dE, v64)
    return h0, e0, t0, np.einsum("bcd,bkd->kbc", err, np.abs(v64)) + D * U * np.einsum("bcd,bkd->kbc", np.abs(dE), np.abs(v64))


def _chain(a, ea, M, n_terms):
    """rules (1) / (4): a M with operand error, an n_terms-term FMA chain"""
    A = np.abs(M)
    return a @ M, ea @ A + n_terms * U * ((np.abs(a) + ea) @ A) + F.FLOOR


def table_bound(g, x, v, hb, ehb, tb, etb):
    """the grid's part: hb [B][IN] = dL/dh_0 and tb [K][B][IN] = dL/dt_0 with their bounds"""
    Fe, D, K = g.n_features_per_level, x.shape[1], v.shape[1]
    n = g.n_levels * Fe
    grad, count, absum, esum, S_level = G.grid_gradient(g, x, (np.abs(hb) + ehb)[:, :n])
    tol = G.gradient_bound(g, grad, count, absum, esum, S_level) + G.grid_gradient(g, x, ehb[:, :n])[0]
    va, smooth = np.abs(v.astype(np.float64)), g.interpolation == 2
    eG = np.einsum("bkd,kbc->bcd", va, etb) + K * U * np.einsum("bkd,kbc->bcd", va, np.abs(tb) + etb)
    aG = np.abs(np.einsum("bkd,kbc->bcd", v.astype(np.float64), tb)) + eG
    tabs, terr = np.zeros(g.n_params), np.zeros(g.n_params)
    for l in range(g.n_levels):
        idx, _, _, dw, SD = corners(g, l, x)
        coef = np.abs(dw)
        ecoef = U * ((2 * (D - 1) + 3 + (3 if smooth else 0)) * coef + 4 * SD)
        for f in range(Fe):
            mag = np.einsum("bcd,bd->bc", coef, aG[:, l * Fe + f])
            np.add.at(tabs, idx * Fe + f, mag)
            np.add.at(terr, idx * Fe + f, np.einsum("bcd,bd->bc", coef, eG[:, l * Fe + f]) + np.einsum("bcd,bd->bc", ecoef, aG[:, l * Fe + f]) + D * U * mag)
    tol_t = terr + count * U * tabs
    return tol + tol_t + U * (grad + tol + tabs + tol_t) + F.FLOOR


def bound(case, enc, g, p, x, v, Cy, CJ):
    """per-element bound of dL/dparams, float64 [n_params]"""
    B, K, NH = x.shape[0], v.shape[1], case.NH
    names = [case.act] * NH + [case.out_act]
    mats = [m.astype(np.float64) for m in F.split(case.W, case.IN, NH, case.OUTP, p[:case.n_mlp])]
    h0, e_h0, t0, e_t0 = encoded(case, enc, g, p, x, v)
    first = F.reference(case.W, case.IN, NH, case.OUTP, case.act, case.out_act, p[:case.n_mlp], h0, Cy, e_x=e_h0)
    h = [h0] + first["hidden"] + [first["out"]]
    eh = [e_h0] + list(first["e_hidden"]) + [first["e_out"]]
    t, et, s, es = [t0], [e_t0], [], []
    for j in range(NH + 1):
        sj, esj = _chain(t[j], et[j], mats[j].T, mats[j].shape[1])
        tj, etj = S2._gate(names[j], sj, esj, h[j + 1], eh[j + 1])
        s, es, t, et = s + [sj], es + [esj], t + [tj], et + [etj]
    hb, ehb = Cy.astype(np.float64), np.zeros(Cy.shape)
    tb = np.zeros((K,) + Cy.shape)
    tb[:, :, :case.n_out] = CJ.astype(np.float64).transpose(2, 0, 1)
    etb = np.zeros_like(tb)
    n_slabs = ((1 + K) * B + F.SLAB_ROWS - 1) // F.SLAB_ROWS
    e_w = [None] * (NH + 1)
    for j in range(NH, -1, -1):
        y, ey = h[j + 1], eh[j + 1]
        sb, esb = S2._gate(names[j], tb, etb, y, ey)
        zb, ezb = S2._gate(names[j], hb, ehb, y, ey)
        if S2.has_curvature(names[j]):
            pr, epr = s[j] * tb, S2._product(s[j], es[j], tb, etb)
            acc, eacc = pr.sum(0), epr.sum(0) + K * U * (np.abs(pr) + epr).sum(0)
            ps = S2.psi(names[j], y)
            c, ec = acc * ps, S2._product(acc, eacc, ps, S2.psi_error(names[j], y, ey))
            zb, ezb = zb + c, ezb + ec + U * (np.abs(zb) + ezb + np.abs(c) + ec)
        Gs, eG = np.concatenate([zb[None], sb]), np.concatenate([ezb[None], esb])
        Xs, eX = np.concatenate([h[j][None], t[j]]), np.concatenate([eh[j][None], et[j]])
        aX = np.abs(Xs) + eX
        e_w[j] = (np.einsum("qbn,qbk->nk", eG, aX) + np.einsum("qbn,qbk->nk", np.abs(Gs), eX) +
                  (F.SLAB_ROWS + n_slabs) * U * np.einsum("qbn,qbk->nk", np.abs(Gs) + eG, aX) + F.FLOOR)
        hb, ehb = _chain(zb, ezb, mats[j], mats[j].shape[0])
        tb, etb = _chain(sb, esb, mats[j], mats[j].shape[0])
    out = np.concatenate([e.ravel() for e in e_w])
    return out if g is None else np.concatenate([out, table_bound(g, x, v, hb, ehb, tb, etb)])
