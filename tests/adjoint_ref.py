"""The adjoint (transpose) of the Green-Gauss gradient in numpy -- test infrastructure, not product, next to the oracle's
np_gradients (oracle/cpu_ref.py), which it is checked against (tests/test_adjoint_oracle.py: the transpose of the dense
matrix built column by column from np_gradients, and the dot-product identity against the compiled reference's golden
gradients).  Operator and exchange argument: DESIGN.md section 11."""
import numpy as np


def np_gradients_adjoint(fpoint, fnormal, pvolume, gbar, nown, ghosts=False):
    """vbar = A^T gbar for the forward map g_own = A var of np_gradients.  With s[p] = gbar[p] / V_p:
        vbar[q][e] = sum_{f in q} 1/2 n_f . (s[p0_f][e] - s[p1_f][e])
    (the same term for both ends of a face).  ghosts = False: s of a ghost point is 0 -- the transpose of the partition's
    own map, every column of it: the rows of ghost points hold d<g_own, gbar>/d var_ghost, which no GPU kernel computes.
    ghosts = True: the caller's ghost rows of gbar (with their pvolume) are the owners' -- the transpose of the global
    operator on the owned rows."""
    fp = np.asarray(fpoint)
    n = np.asarray(fnormal, np.float64)
    s = np.asarray(gbar, np.float64) / np.asarray(pvolume, np.float64)[:, None, None]
    if not ghosts:
        s = s.copy()
        s[nown:] = 0.0
    d = 0.5 * np.einsum("fd,fed->fe", n, s[fp[:, 0]] - s[fp[:, 1]])
    vbar = np.zeros((len(pvolume), 7))
    np.add.at(vbar, fp[:, 0], d)
    np.add.at(vbar, fp[:, 1], d)
    return vbar


def np_adjoint_scale(fpoint, fnormal, pvolume, gbar, nown, ghosts=False):
    """sum |terms| of every vbar component: sum_{f in q} 1/2 sum_d |n_f[d]| (|s[p0][e][d]| + |s[p1][e][d]|) -- the scale
    a cancelling sum is judged against (the adjoint's counterpart of np_scale)"""
    fp = np.asarray(fpoint)
    n = np.abs(np.asarray(fnormal, np.float64))
    s = np.abs(np.asarray(gbar, np.float64) / np.asarray(pvolume, np.float64)[:, None, None])
    if not ghosts:
        s = s.copy()
        s[nown:] = 0.0
    d = 0.5 * np.einsum("fd,fed->fe", n, s[fp[:, 0]] + s[fp[:, 1]])
    out = np.zeros((len(pvolume), 7))
    np.add.at(out, fp[:, 0], d)
    np.add.at(out, fp[:, 1], d)
    return out


def dense_gradient_matrix(np_gradients, fpoint, fnormal, pvolume, nown):
    """A [(nown * 21) x (nall * 7)]: column j = the owned rows of np_gradients of the unit var e_j"""
    nall = len(pvolume)
    cols = []
    for j in range(nall * 7):
        v = np.zeros((nall, 7))
        v.flat[j] = 1.0
        cols.append(np_gradients(fpoint, fnormal, pvolume, v, nown)[:nown].ravel())
    return np.stack(cols, 1)
