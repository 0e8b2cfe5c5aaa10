"""QuatMpc's problem with a CONTACT SCHEDULE over the horizon (qmpc_solve_schedule*), restated on top of
tests/kkt_independent.py -- no code shared with oracle/ or with the HIP kernels.

`masks` [N] (uint8, bit l: leg l stands during knot k) replaces the record's contacts[4]:
  * a leg in the air at a knot carries zero force there and is no variable there
  * the cone rows of a (knot, leg) exist only where the bit is set
  * u_ref_k[3l+2] = c_kl mass 9.81 / nc_k, nc_k the number of legs standing at knot k (QuatMpc.cpp:121-125 per knot)
  * dynamics, state cost, attitude cost, foot positions (one per leg for the whole horizon) and references are QuatProblem's

ScheduleProblem overrides exactly what the stance set enters (the mask of the rollout, the input term of the cost, the mask of
the gradient).  The certificate and the independent solver are kkt_independent's own, kkt_residuals and active_set_newton, applied
to a VIEW of the problem as one knot with 4 N legs: (knot, leg) pairs are then that module's legs, and "stance" is the pair's bit.
"""
from __future__ import annotations

import numpy as np
import torch

import kkt_independent as K


def mask_bits(masks, nl: int = 4) -> np.ndarray:
    """[N] uint8 -> [N][nl] 0.0 / 1.0"""
    m = np.asarray(masks, dtype=np.int64)
    return ((m[:, None] >> np.arange(nl)[None, :]) & 1).astype(float)


class ScheduleProblem(K.QuatProblem):
    """One QuatMpc instance whose stance set is given per knot.  The record's contacts are not read."""

    def __init__(self, par, rec, masks):
        super().__init__(par, _with_contacts(rec, np.ones(4)))      # (the base class's own u_ref and mask are replaced below)
        con = mask_bits(masks, self.nl)
        if con.shape != (self.N, self.nl):
            raise ValueError(f"masks: {con.shape}, expected ({self.N}, {self.nl})")
        if (con.sum(1) == 0).any():
            raise ValueError("a knot without a stance leg (flight phases are out of scope)")
        self.conk = con                                              # [N][nl]
        self.maskk = torch.tensor(np.repeat(con, 3, axis=1))         # [N][nu]
        urefk = np.zeros((self.N, self.nu))
        for k in range(self.N):
            nc = int(con[k].sum())
            urefk[k, 2::3] = con[k] * self.mass * K.GRAV / nc        # QuatMpc.cpp:121-125, per knot
        self.urefk = torch.tensor(urefk)
        # what the base class derived from contacts[4] must not be used any more
        self.con = self.uref = self.mask = None

    def rollout(self, U, project=True):
        X = [self.x0]
        for k in range(self.N):
            xn = self.step(X[-1], U[k] * self.maskk[k])
            X.append(K.TangentProject.apply(xn) if project else xn)
        return X

    def cost(self, X, U):
        J = 0.0
        for k in range(self.N + 1):
            e = X[k] - self.xref[k]
            J = J + 0.5 * (self.Q * e * e).sum() + self.w * (1.0 - torch.abs(torch.dot(self.xref[k, 3:7], X[k][3:7])))
            if k < self.N:
                d = U[k] * self.maskk[k] - self.urefk[k]
                J = J + 0.5 * (self.Rw * d * d).sum()
        return J

    def value_and_grad(self, U_np, project=True):
        U = torch.tensor(np.asarray(U_np, dtype=float).reshape(self.N, self.nu), requires_grad=True)
        J = self.cost(self.rollout(U, project), U)
        (g,) = torch.autograd.grad(J, U)
        return float(J.detach()), g.numpy() * np.repeat(self.conk, 3, axis=1)

    def flat(self):
        return _FlatView(self)

    def kkt(self, U, lam=None):
        """kkt_residuals over the (knot, leg) pairs: stationarity (with `lam` [N][24], zeros when None), stationarity_nnls with
        re-derived multipliers, violation, swing_force = max |u| over the pairs whose bit is clear."""
        U = np.asarray(U, dtype=float).reshape(self.N, self.nu)
        _, g = self.value_and_grad(U)
        lam = np.zeros((self.N, 6 * self.nl)) if lam is None else np.asarray(lam, dtype=float)
        return K.kkt_residuals(g.reshape(1, -1), U.reshape(1, -1), lam.reshape(1, -1), self.frame(), self.conk.ravel(), self.mu,
                               self.fz_max)

    def active_rows(self, U, tol=1e-6) -> int:
        """cone rows of standing (knot, leg) pairs with slack <= tol"""
        _, c = K.cone_rows(np.asarray(U, dtype=float).reshape(1, -1), self.frame(), self.conk.ravel(), self.mu, self.fz_max)
        return int((-c[0][self.conk.ravel() != 0] <= tol).sum())


def _with_contacts(rec, con):
    r = np.zeros(1, dtype=rec.dtype)      # (a record taken out of an array is a view of it: np.array(rec) would still share its bytes)
    r[0] = rec
    r["contacts"][0] = con
    return r[0]


class _FlatView:
    """The scheduled problem as kkt_independent sees a problem: ONE knot, 4 N legs, stance = the pair's bit."""

    def __init__(self, p: ScheduleProblem):
        self.p = p
        self.N, self.nu, self.nl = 1, p.N * p.nu, p.N * p.nl
        self.con = p.conk.ravel()
        self.uref = p.urefk.numpy().ravel()
        self.mu, self.fz_max = p.mu, p.fz_max

    def frame(self):
        return self.p.frame()

    def value_and_grad(self, U):
        J, g = self.p.value_and_grad(np.asarray(U).reshape(self.p.N, self.p.nu))
        return J, g.reshape(1, -1)


def active_set_newton_schedule(prob: ScheduleProblem, iters=400, tol=1e-10):
    """kkt_independent.active_set_newton on the per-knot stance variables, from U = u_ref_k.  Returns (U [N][12], working set,
    multipliers, iterations); a working-set entry is 6 j + i for row i of the j-th standing (knot, leg) pair in knot-major order."""
    U, W, lam, it = K.active_set_newton(prob.flat(), iters=iters, tol=tol)
    return U.reshape(prob.N, prob.nu), W, lam, it
