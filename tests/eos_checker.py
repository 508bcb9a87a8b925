"""An independent numpy restatement of cooling_fine in a barotropic run of constant temperature without cooling
(hydro/cooling_fine.f90:162-181, 264-308, 331-347, 537-540, 563-566, 576-579), NDIM = 3, NENER = 0, SOLVER=hydro.

numpy evaluates every binary operation on float64 arrays as one correctly rounded IEEE operation, so an expression written in the
reference's order carries the reference's bits.  tests/test_eos_checker.py holds this file to records of the reference program;
the device tests then compare with it at tolerance zero."""
import numpy as np


def energy(rho, mx, my, mz, T2c, scale_nH, scale_T2, smallr, gamma):
    """the new uold(:,5) of leaf cells"""
    nH = np.maximum(rho, smallr)
    ekk = np.zeros_like(nH)
    for m in (mx, my, mz):                       # idim = 2..4, left to right
        ekk = ekk + 0.5 * m ** 2 / nH
    nHcc = nH * scale_nH                         # into H/cc ...
    nH2 = nHcc / scale_nH                        # ... and back: not the identity
    e = T2c * nH2 / scale_T2 / (gamma - 1.0)
    return e + ekk + 0.0 + 0.0                   # + err + emag


def cooling_fine(u, son, T2c, scale_nH, scale_T2, smallr, gamma):
    """u[nvar][n] and son[n] of any set of cells -> the state after cooling_fine: variable 5 of the leaf cells rewritten"""
    out = u.copy()
    leaf = son == 0
    out[4, leaf] = energy(u[0, leaf], u[1, leaf], u[2, leaf], u[3, leaf], T2c, scale_nH, scale_T2, smallr, gamma)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
