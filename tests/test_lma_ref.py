"""The derivation of the low-mode averaged scalar trace, held in dense algebra on 4^4 (no GPU): with P the projector of
tests/lma_ref.py on 16 dense eigenvectors, Q = 1 - P and M = D + m,

    L(x) + m sum_y |(Q M^-1)(x, y)|^2 = m (M^+ M)^-1(x, x)          the noise expectation of the improved estimator
    L(x) + sum_col (Q M^-1)(x col, x col) = m (M^+ M)^-1(x, x)      and of the unimproved one

on every site of both parities; with all 384 modes Q M^-1 = 0 and L is the whole diagonal; both sum rules.  A wrong weight, a wrong
sign in the odd projector or a missing 1/lambda breaks these identities at O(1).

Bar 1e-11 of max L: the condition number of M^+ M is below 100 and the sums have 384 terms, so about 1e-13 is expected."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import eig_ref as E  # noqa: E402
import lma_ref as LR  # noqa: E402

LAT = (4, 4, 4, 4)
MASS = 0.1
BAR = 1e-11


@pytest.fixture(scope="module")
def A():
    _, w, v = E.dense(LAT)
    D = LR.dense_D(LAT)
    n2 = D.shape[0]
    assert w.shape == (384,) and w[0] > 0
    assert np.abs(D + D.conj().T).max() == 0.0
    M = D + MASS * np.eye(n2)
    Minv = np.linalg.inv(M)
    full = MASS * np.linalg.inv(M.conj().T @ M)
    print("cond(M^+ M) = %.1f" % np.linalg.cond(M.conj().T @ M))
    return dict(w=w, v=v, D=D, Minv=Minv, want=np.diag(full).real.reshape(-1, 3).sum(axis=1), mul=lambda X: D @ X)


def _site(d):
    return np.asarray(d).reshape(-1, 3).sum(axis=1)


@pytest.mark.parametrize("nev", [16, 384])
def test_both_estimators_have_the_exact_expectation(A, nev):
    proj = LR.Projector(A["v"][:, :nev], A["w"][:nev], A["mul"])
    L = proj.diag(MASS)
    scale = L.max()
    QMinv = proj.Q(A["Minv"])
    imp = L + MASS * _site((np.abs(QMinv) ** 2).sum(axis=1))
    dq = np.diag(QMinv)
    unimp = L + _site(dq.real)
    d1, d0, di = np.abs(imp - A["want"]).max() / scale, np.abs(unimp - A["want"]).max() / scale, np.abs(_site(dq.imag)).max() / scale
    print("nev = %d: improved %.3e, unimproved %.3e, Im %.3e of max L = %.6g" % (nev, d1, d0, di, scale))
    assert L.shape == (256,) and d1 < BAR and d0 < BAR and di < BAR
    if nev == 384:
        dl, dm = np.abs(L - A["want"]).max() / scale, np.abs(QMinv).max()
        print("complete basis: |L - diag| %.3e of max L, max|Q M^-1| %.3e" % (dl, dm))
        assert dl < BAR and dm < BAR
    else:
        assert np.abs(QMinv).max() > 0.1 and (L < A["want"]).all()         # the remainder is not small, and positive


@pytest.mark.parametrize("nev", [16, 384])
def test_sum_rules(A, nev):
    lam = A["w"][:nev]
    proj = LR.Projector(A["v"][:, :nev], lam, A["mul"])
    L = proj.diag(MASS)
    want = (MASS / (MASS * MASS + lam)).sum()
    de, do = abs(L[:128].sum() - want) / want, abs(L[128:].sum() - want) / want
    print("nev = %d: sum rules even %.3e odd %.3e of %.6g" % (nev, de, do, want))
    assert de < BAR and do < BAR


def test_P_is_an_orthogonal_projector_that_commutes_with_D(A):
    proj = LR.Projector(A["v"][:, :16], A["w"][:16], A["mul"])
    P = proj.P(np.eye(A["D"].shape[0]))
    assert np.abs(P - P.conj().T).max() < 1e-13 and np.abs(P @ P - P).max() < 1e-13
    assert abs(np.trace(P).real - 32) < 1e-11
    assert np.abs(P @ A["D"] - A["D"] @ P).max() < 1e-12
    # the oracle's operator applied column by column is the dense D
    X = np.random.default_rng(5).standard_normal((A["D"].shape[0], 2)) + 0j
    assert np.abs(LR.oracle_D(LAT)(X) - A["D"] @ X).max() < 1e-13
