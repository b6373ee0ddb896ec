"""Shared by tests/test_adam_host.py and tests/test_gpu_adam.py (not collected): the parameter
list of the kernel tests (tests/_clip_cases.py's Layout, four buffers of it), an fp64 Adam /
AdamW step, a numpy fp32 restatement of the operation order csrc/adam.hip's header states (with
and without fused multiply-adds) and the per-element error bounds both files hold the kernel to.

The bound (derived, not tuned).  U = 2^-24; g_k = (1 + U)^k - 1.  The reference is one step in
fp64 on the same fp32 inputs; everything below is per element.  Exact quantities in capitals:

    G = g + wd p (L2) | g          A = |g| + wd |p| (L2) | |g|       (A >= |G|)
    M = m + c1 (G - m)             c1 = 1 - beta1
    V = beta2 v + c2 G^2           c2 = 1 - beta2
    P1 = p (1 - lr wd) (decoupled) | p
    R = sqrt(V) / sqrt(bc2) + eps,  Q = M / R,  S = lr / bc1,  P = P1 - S Q

adam.hip rounds each fp64 scalar (c1, beta2, c2, eps, wd, 1 - lr wd, S, sqrt(bc2)) to fp32 once
and then runs, one rounding per line:  [g = fma(wd, p, g)]; d = g - m; m = fma(c1, d, m);
a = beta2 v; gg = g g; v = fma(c2, gg, a); [p = p keep]; r = sqrt(v); r = r / bc2s; r = r + eps;
u = m / r; p = fma(-S, u, p).  A build without fused multiply-adds rounds each product once more;
the counts below cover both.

  g (L2): the constant, the product (no fma) and the sum round:   eg = U A + g_3 wd |p|
  m can cancel, so its bound is absolute:  d is within ed = eg + U (A + eg + |m|) of G - m and
      |d| <= Dm = (A + eg + |m|)(1 + U); the constant and the product (no fma) round, then the sum:
      em = c1 ed + c1 g_2 Dm + U (|m| + c1 (1 + U)^2 Dm)
  v is a sum of non-negative terms, so its bound is relative: beta2 v passes 3 roundings
      (constant, product, sum), c2 g^2 passes 4 (gg, constant, product without fma, sum), and
      g^2 is within eG2 = 2 |G| eg + eg^2 of G^2:
      ev = g_4 V + (1 + g_4) c2 eG2
  the denominator, again non-negative terms: sqrt moves an absolute error ev to ev / sqrt(V)
      (V = 0: sqrt(ev)) and rounds; the division by fl(sqrt(bc2)) is within rho = (1 + U) / (1 - U)
      - 1; eps is rounded and the sum rounds:
      es = ev / sqrt(V) + U (sqrt(V) + ev / sqrt(V))
      e2 = es (1 + rho) / B + rho sqrt(V) / B,   B = sqrt(bc2)
      eR = e2 + U eps + U (R + e2 + U eps)                       (the tests assert eR < R)
  the quotient:  eq = em / (R - eR) + |M| eR / (R (R - eR)), then one rounding:
      eq <- eq + U (|Q| + eq)
  p inherits S times that, plus its own roundings: e1 = g_2 |P1| (decoupled: the constant and
      the product; else 0); S and the product (no fma) round, then the sum:
      eu = S (1 + U)^2 eq + g_2 S |Q|
      ep = e1 + eu + U (|P1| + e1 + S |Q| + eu)

The fp64 reference and the kernel's fp64 scalars (pow, sqrt, cos) are within REF = 64 * 2^-53 of
the exact values; REF times the magnitudes (|m| + A, V, |P1| + S |Q|) is added to each bound.

Gradients have |g| >= 1e-3 and lr = 1e-2: the first step of a tensor moves every element by
about lr, orders of magnitude above ep (asserted in test_adam_host.py), so an element updated
zero times or twice cannot pass."""
import os

import numpy as np

import _clip_cases as cc
from conftest import PKG

U, U64, REF = cc.U, cc.U64, cc.REF
C = cc.C
SENTINEL = cc.SENTINEL

LR = 1e-2
BETAS = (0.9, 0.999)
EPS = 1e-8
MODES = {"adam": dict(weight_decay=0.0, decoupled=True),
         "decoupled": dict(weight_decay=0.1, decoupled=True),
         "l2": dict(weight_decay=0.1, decoupled=False)}
OLD = 1000      # preset step count of every second tensor

SRC = open(os.path.join(PKG, "csrc", "adam.hip")).read()


def gamma(k):
    return (1.0 + U) ** k - 1.0


class Case:
    """p, m, v, g over one Layout: four fp32 buffers with the same offsets and SENTINEL guard
    bands.  Tensors with an even index are new (count 0, zero moments), the others have
    count OLD and moments of the gradient's scale."""

    def __init__(self, seed=7):
        self.L = L = cc.Layout()
        rng = np.random.default_rng(seed)
        n = L.size
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
        g = np.where(g < 0, -1.0, 1.0) * np.maximum(np.abs(g), 1e-3)
        p = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2, n)
        self.tensor = np.full(n, -1, np.int64)          # element -> tensor, -1 in the guards
        for i, (o, k) in enumerate(zip(L.offsets, L.numels)):
            self.tensor[o:o + k] = i
        self.mask = L.mask
        self.counts = np.where(np.arange(len(L.numels)) % 2 == 0, 0, OLD).astype(np.int64)
        old = self.mask & (self.counts[self.tensor] == OLD)
        a = rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)
        b = rng.uniform(0.5, 1.5, n)
        m = np.where(old, g * a, 0.0)
        v = np.where(old, g * g * b, 0.0)
        self.p, self.m, self.v, self.g = (self._buf(x) for x in (p, m, v, g))
        self.t = np.where(self.mask, self.counts[self.tensor] + 1, 1).astype(np.float64)

    def _buf(self, x):
        out = np.full(self.L.size, SENTINEL, np.float32)
        out[self.mask] = x.astype(np.float32)[self.mask]
        return out

    def listed(self, leave_out=()):
        """Element mask of the tensors a step lists."""
        keep = np.ones(len(self.L.numels), bool)
        keep[list(leave_out)] = False
        return self.mask & keep[self.tensor]


def _scalars(t, lr, betas, eps):
    bc1 = 1.0 - betas[0] ** t
    bc2 = 1.0 - betas[1] ** t
    return lr / bc1, np.sqrt(bc2)


def reference(p, m, v, g, t, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=True):
    """One step in fp64 on fp32 (or fp64) inputs: (P, M, V) and the intermediate magnitudes the
    bound needs."""
    p, m, v, g = (np.asarray(x, np.float64) for x in (p, m, v, g))
    l2 = weight_decay != 0.0 and not decoupled
    G = g + weight_decay * p if l2 else g
    A = np.abs(g) + weight_decay * np.abs(p) if l2 else np.abs(g)
    c1, c2 = 1.0 - betas[0], 1.0 - betas[1]
    M = m + c1 * (G - m)
    V = betas[1] * v + c2 * G * G
    P1 = p * (1.0 - lr * weight_decay) if (weight_decay != 0.0 and decoupled) else p
    S, B = _scalars(t, lr, betas, eps)
    R = np.sqrt(V) / B + eps
    Q = M / R
    P = P1 - S * Q
    return P, M, V, dict(G=G, A=A, P1=P1, S=S, B=B, R=R, Q=Q)


def bounds(p, m, v, g, t, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=True):
    """(ep, em, ev): per-element absolute bounds on |kernel - fp64| (the module docstring)."""
    P, M, V, x = reference(p, m, v, g, t, lr, betas, eps, weight_decay, decoupled)
    p, m = np.abs(np.asarray(p, np.float64)), np.abs(np.asarray(m, np.float64))
    G, A, P1, S, B, R, Q = (x[k] for k in ("G", "A", "P1", "S", "B", "R", "Q"))
    c1, c2 = 1.0 - betas[0], 1.0 - betas[1]
    l2 = weight_decay != 0.0 and not decoupled
    eg = U * A + gamma(3) * weight_decay * p if l2 else np.zeros_like(A)
    ed = eg + U * (A + eg + m)
    Dm = (A + eg + m) * (1 + U)
    em = c1 * ed + c1 * gamma(2) * Dm + U * (m + c1 * (1 + U) ** 2 * Dm)
    eG2 = 2 * np.abs(G) * eg + eg * eg
    ev = gamma(4) * V + (1 + gamma(4)) * c2 * eG2
    rootV = np.sqrt(V)
    with np.errstate(divide="ignore", invalid="ignore"):
        moved = np.where(V > 0, ev / rootV, np.sqrt(ev))
    es = moved + U * (rootV + moved)
    rho = (1 + U) / (1 - U) - 1
    e2 = es * (1 + rho) / B + rho * rootV / B
    eR = e2 + U * eps + U * (R + e2 + U * eps)
    assert (eR < R).all()
    eq = em / (R - eR) + np.abs(M) * eR / (R * (R - eR))
    eq = eq + U * (np.abs(Q) + eq)
    dec = weight_decay != 0.0 and decoupled
    e1 = gamma(2) * np.abs(P1) if dec else np.zeros_like(P1)
    eu = S * (1 + U) ** 2 * eq + gamma(2) * S * np.abs(Q)
    ep = e1 + eu + U * (np.abs(P1) + e1 + S * np.abs(Q) + eu)
    em = em + REF * (m + A)
    ev = ev + REF * V
    ep = ep + REF * (np.abs(P1) + S * np.abs(Q))
    return ep, em, ev


# ------------------------------------------------------------------ fp32 restatement
def _f(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _fma(a, b, c, fused):
    """fl32(a b + c) for fp32 arrays: the product of two fp32 values is exact in fp64, so the
    fused form differs from one fp32 rounding only in a double-rounding tie, far below the
    bound's slack; the unfused form rounds the product to fp32 first."""
    prod = a.astype(np.float64) * b.astype(np.float64)
    if not fused:
        prod = prod.astype(np.float32).astype(np.float64)
    return (prod + c.astype(np.float64)).astype(np.float32)


def emulate(p, m, v, g, t, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled=True,
            fused=True):
    """(p, m, v) in fp32 in the operation order adam.hip's header states."""
    p, m, v, g = (np.asarray(x, np.float32) for x in (p, m, v, g))
    S, B = _scalars(np.asarray(t, np.float64), lr, betas, eps)
    one = np.ones_like(p)
    omb1, b2, omb2 = (_f(x) * one for x in (1.0 - betas[0], betas[1], 1.0 - betas[1]))
    epsf, wdf, keep = _f(eps) * one, _f(weight_decay) * one, _f(1.0 - lr * weight_decay) * one
    step, bc2s = _f(S) * one, _f(B) * one
    if weight_decay != 0.0 and not decoupled:
        g = _fma(wdf, p, g, fused)
    d = (g - m).astype(np.float32)
    m = _fma(omb1, d, m, fused)
    a = (b2 * v).astype(np.float32)
    gg = (g * g).astype(np.float32)
    v = _fma(omb2, gg, a, fused)
    if weight_decay != 0.0 and decoupled:
        p = (p * keep).astype(np.float32)
    r = np.sqrt(v).astype(np.float32)
    r = (r / bc2s).astype(np.float32)
    r = (r + epsf).astype(np.float32)
    u = (m / r).astype(np.float32)
    p = _fma(-step, u, p, fused)
    return p, m, v


def worst_ratio(got, want, bound, mask):
    """max over the masked elements of |got - want| / bound."""
    err = np.abs(np.asarray(got, np.float64) - want)[mask]
    return float(np.max(err / bound[mask]))
