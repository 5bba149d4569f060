"""NumPy restatement of include/kdehip.h section 5m, written from its text: evaluation within a tolerance by pruning the
all-pairs sum on the density's 128-leaf chunks.  Everything takes LEAF-ORDER arrays: `pts` (N, D) leaf centres, `w` (N,)
leaf weights, `v` (D,) variances, `qry` (Nq, D) queries in the order they are processed (leave-one-out: qry is pts).  The
model's arithmetic is numpy's (no fused multiply-add), so it agrees with the device to rounding, not to the bit; what it pins
is the rule: boxes, L_q, tau_q, the flags and the restricted sum."""
import math

import numpy as np

CHUNK, BLOCK = 128, 256
MARGIN = 2.0 ** -20
CIRC_FAR = math.pi * (1.0 + 2.0 ** -20)


def wrap(d):
    return d - 2.0 * math.pi * np.floor((d + math.pi) / (2.0 * math.pi))


def exponents(pts, v, qry, circ=()):
    """a[q, i] = -1/2 sum_k diff_k(x_qk, c_ik)^2 / v_k, k ascending"""
    a = np.zeros((qry.shape[0], pts.shape[0]))
    for k in range(pts.shape[1]):
        d = qry[:, k, None] - pts[None, :, k]
        if k in circ:
            d = wrap(d)
        a += d * d * (-0.5 / v[k])
    return a


def norm(v):
    out = (2.0 * math.pi) ** (len(v) / 2.0)
    for x in v:
        out *= math.sqrt(x)
    return out


def boxes(pts, w):
    """step 1: lo (nc, D), hi (nc, D), W (nc,)"""
    N = pts.shape[0]
    nc = (N + CHUNK - 1) // CHUNK
    lo = np.stack([pts[c * CHUNK:(c + 1) * CHUNK].min(axis=0) for c in range(nc)])
    hi = np.stack([pts[c * CHUNK:(c + 1) * CHUNK].max(axis=0) for c in range(nc)])
    W = np.array([sum(w[c * CHUNK:(c + 1) * CHUNK].tolist(), 0.0) for c in range(nc)])
    return lo, hi, W


def bounds(lo, hi, v, qry, circ=()):
    """step 2: a_min, a_max (Nq, nc)"""
    amin = np.zeros((qry.shape[0], lo.shape[0]))
    amax = np.zeros_like(amin)
    for k in range(lo.shape[1]):
        below, above = lo[None, :, k] - qry[:, k, None], qry[:, k, None] - hi[None, :, k]
        dmin = np.maximum(0.0, np.maximum(below, above))
        dmax = np.maximum(np.abs(below), np.abs(above))
        if k in circ:
            dmin, dmax = np.zeros_like(dmin), np.full_like(dmax, CIRC_FAR)
        amin += dmin * dmin * (-0.5 / v[k])
        amax += dmax * dmax * (-0.5 / v[k])
    return amin, amax


def _plan_block(pts, w, v, qry, q0, box, rel_tol, abs_tol, loo, circ):
    """steps 2-4 for the queries q0 .. q0 + len(qry) - 1 of ONE block, and their terms T[q, i] = w_i exp(a_qi) (0 for the
    own leaf in leave-one-out)"""
    lo, hi, W = box
    n, nc = qry.shape[0], lo.shape[0]
    idx = np.arange(n)
    with np.errstate(invalid="ignore"):
        amin, amax = bounds(lo, hi, v, qry, circ)
        T = w[None, :] * np.exp(exponents(pts, v, qry, circ))
    far = W[None, :] * np.exp(amax)
    if loo:
        T[idx, q0 + idx] = 0.0
        far[idx, (q0 + idx) // CHUNK] = 0.0
    far = far.sum(axis=1)
    live = ~np.isnan(qry).any(axis=1)
    L, tau = np.zeros(n), np.zeros(n)
    need = np.zeros((n, nc), dtype=bool)
    for q in np.nonzero(live)[0]:
        cstar = int(np.argmax(amin[q]))  # (the first of equal maxima: the lowest c)
        near = sum(T[q, cstar * CHUNK:(cstar + 1) * CHUNK].tolist(), 0.0)
        L[q] = max(far[q], near)
        tau[q] = max(rel_tol * L[q], abs_tol * norm(v))
        need[q] = True if tau[q] == 0.0 else amin[q] > math.log(tau[q]) - MARGIN
    return dict(L=L, tau=tau, need=need, visited=need.any(axis=0), T=T, live=live)


def plan(pts, w, v, qry, rel_tol, abs_tol, loo=False, circ=()):
    """steps 1-4: dict with L (Nq,), tau (Nq,), need (Nq, nc) bool and visited (qblocks, nc) bool"""
    box = boxes(pts, w)
    blocks = [_plan_block(pts, w, v, qry[q0:q0 + BLOCK], q0, box, rel_tol, abs_tol, loo, circ)
              for q0 in range(0, qry.shape[0], BLOCK)]
    out = {k: np.concatenate([b[k] for b in blocks]) for k in ("L", "tau", "need", "live")}
    out["visited"] = np.stack([b["visited"] for b in blocks])
    return out


def evaluate_tol(pts, w, v, qry, rel_tol, abs_tol, loo=False, circ=()):
    """step 5: (p_hat (Nq,) in processing order, (tiles visited, tiles in all)): per query the sums of the visited chunks of
    its block, added in chunk order (the device adds them group by group: the same terms, another association)"""
    box = boxes(pts, w)
    nc = box[0].shape[0]
    out, visited = [], 0
    for q0 in range(0, qry.shape[0], BLOCK):
        b = _plan_block(pts, w, v, qry[q0:q0 + BLOCK], q0, box, rel_tol, abs_tol, loo, circ)
        s = np.zeros(b["T"].shape[0])
        for c in np.nonzero(b["visited"])[0]:
            s = s + b["T"][:, c * CHUNK:(c + 1) * CHUNK].sum(axis=1)
        s = s / norm(v)
        if loo:
            s = s / (1.0 - w[q0:q0 + s.shape[0]])
        s[~b["live"]] = math.nan
        out.append(s)
        visited += int(b["visited"].sum())
    return np.concatenate(out), (visited, len(out) * nc)


def direct_fsum(pts, w, v, qry, loo=False, circ=()):
    """the full sum, one math.fsum per query: the reference of the model's own bound"""
    out = np.zeros(qry.shape[0])
    for q0 in range(0, qry.shape[0], BLOCK):
        T = w[None, :] * np.exp(exponents(pts, v, qry[q0:q0 + BLOCK], circ))
        if loo:
            idx = np.arange(T.shape[0])
            T[idx, q0 + idx] = 0.0
        out[q0:q0 + T.shape[0]] = [math.fsum(row.tolist()) for row in T]
    out /= norm(v)
    return out / (1.0 - w) if loo else out
