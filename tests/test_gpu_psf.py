"""`ort_psf_f64`: diffraction PSF and Strehl ratio of Zernike wavefronts on the device, against the definition evaluated by
numpy in complex128 — W from the explicit factorial formula of R_n^m, the double sum as `Ey @ P @ Ex.T`.  No code shared with
the kernel's recurrences or its matrix product.  Bound 1e-11 absolute on values <= 1: the float64 reference lies within
4.5e-16 of a long-double direct sum; the kernel's recurrences hold 1e-14 relative on |W| <= 10 waves, a coherent phase error of
at most 2 pi 1e-13, so <= 2e-12 on the PSF."""
from math import factorial, sqrt

import numpy as np
import pytest

import opticalraytracing_jl_amd as ort
from opticalraytracing_jl_amd import _capi
from tests import common as cm

pytestmark = pytest.mark.gpu
TOL = 1e-11


def reference_psf(coef, degree, npupil, nimg, dxi, centre):
    """[nb][nimg][nimg] from coef [nb][nterms] and centre [nb][2]: the definition in include/ort.h, term by term."""
    x = (2.0 * np.arange(npupil) + 1.0 - npupil) / npupil
    X, Y = np.meshgrid(x, x)                                          # X[j][k] = x_k, Y[j][k] = y_j
    mask, rho, theta = X * X + Y * Y <= 1.0, np.hypot(X, Y), np.arctan2(Y, X)
    Z = []
    for n, m in ort.zernike_terms(degree):
        mu, R = abs(m), np.zeros_like(rho)
        for k in range((n - mu) // 2 + 1):
            R += (-1) ** k * factorial(n - k) / (factorial(k) * factorial((n + mu) // 2 - k) * factorial((n - mu) // 2 - k)) * rho ** (n - 2 * k)
        Z.append(sqrt(2 * (n + 1) / (2 if m == 0 else 1)) * R * (np.cos(mu * theta) if m >= 0 else np.sin(mu * theta)))
    W = np.tensordot(np.asarray(coef, dtype=np.float64), np.array(Z), axes=1)
    P = mask * np.exp(2j * np.pi * W)
    m = (np.arange(nimg) - nimg // 2) * dxi
    centre = np.asarray(centre, dtype=np.float64)
    Ex = np.exp(-2j * np.pi * (centre[:, 0, None, None] + m[None, :, None]) * x)      # [nb][nimg][npupil]
    Ey = np.exp(-2j * np.pi * (centre[:, 1, None, None] + m[None, :, None]) * x)
    return np.abs(Ey @ P @ Ex.transpose(0, 2, 1)) ** 2 / mask.sum() ** 2


def wavefronts(rng, nb, degree, rms):
    """Random coefficient rows scaled to the given wavefront RMS in waves (the terms are orthonormal)."""
    c = rng.normal(size=(nb, len(ort.zernike_terms(degree))))
    return c / np.linalg.norm(c, axis=1, keepdims=True) * np.reshape(rms, (-1, 1))


@pytest.mark.parametrize("npupil,nimg,degree", ((32, 16, 1), (32, 16, 4), (48, 48, 10), (80, 16, 7), (32, 128, 5)))
def test_psf_matches_direct_sum(hip_engine, npupil, nimg, degree):
    """One and several image tiles, the register cap (nimg = 128), pupils that are no multiple of 32 or 64, and 80 = 5 panels:
    three bundles are cut into spans and folded.  Bundle 2 has no fit."""
    import torch
    rng = np.random.default_rng(31000 + npupil + nimg + degree)
    dxi, centre, info = 0.125, np.array([[0.0, 0.0], [0.3, -0.2], [0.0, 0.0]]), np.array([0, 0, 1], dtype=np.int32)
    coef = wavefronts(rng, 3, degree, [0.1, 1.0, 3.0])
    coef[2] = np.nan
    want = reference_psf(coef[:2], degree, npupil, nimg, dxi, centre[:2])
    psf, strehl = hip_engine.psf(coef, degree, npupil, nimg, dxi, centre=centre, info=info)
    dev = max(np.abs(psf[:2] - want).max(), np.abs(strehl[:2] - want[:, nimg // 2, nimg // 2]).max())
    print(f"psf ({npupil}, {nimg}, {degree}): worst deviation {dev:.3e}, strehl {strehl[0]:.6f} {strehl[1]:.3e}")
    cm.report(f"psf npupil {npupil} nimg {nimg} degree {degree}: worst deviation from the direct sum {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL
    assert np.isnan(psf[2]).all() and np.isnan(strehl[2])
    assert np.array_equal(strehl, psf[:, nimg // 2, nimg // 2], equal_nan=True)
    none, only = hip_engine.psf(coef, degree, npupil, nimg, dxi, centre=centre, info=info, want_psf=False)
    assert none is None and np.array_equal(only, strehl, equal_nan=True)
    dv = torch.device("cuda:0")
    d = [torch.from_numpy(a).to(dv) for a in (coef, centre, info)]
    torch.cuda.synchronize(dv)
    runs = [hip_engine.psf(d[0], degree, npupil, nimg, dxi, centre=d[1], info=d[2]) for _ in range(2)]
    runs.append((runs[0][0], hip_engine.psf(d[0], degree, npupil, nimg, dxi, centre=d[1], info=d[2], want_psf=False)[1]))
    hip_engine.ctx.synchronize()
    for dp, ds in runs:                                               # device pointers == host pointers, and run to run
        assert np.array_equal(dp.cpu().numpy(), psf, equal_nan=True) and np.array_equal(ds.cpu().numpy(), strehl, equal_nan=True)


def test_many_bundles_route(hip_engine):
    """1200 bundles exceed four workgroups per compute unit: one workgroup per bundle, written without a workspace.  Every
    bundle has its own coefficients and centre, so a slot or index mix-up between bundles fails."""
    rng = np.random.default_rng(31415)
    nb, npupil, nimg, degree, dxi = 1200, 32, 16, 4, 0.125
    coef, centre = wavefronts(rng, nb, degree, rng.uniform(0.05, 1.0, size=nb)), rng.uniform(-0.5, 0.5, size=(nb, 2))
    want = reference_psf(coef, degree, npupil, nimg, dxi, centre)
    psf, strehl = hip_engine.psf(coef, degree, npupil, nimg, dxi, centre=centre)
    dev = np.abs(psf - want).max()
    cm.report(f"psf, 1200 bundles: worst deviation from the direct sum {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL
    assert np.array_equal(strehl, psf[:, nimg // 2, nimg // 2])
    assert np.array_equal(hip_engine.psf(coef, degree, npupil, nimg, dxi, centre=centre, want_psf=False)[1], strehl)


def test_conventions(hip_engine):
    """Sign, wavegrad unit and N^2 normalisation, independently of the reference function: a flat wavefront peaks at exactly 1;
    a tilt a Z_1^1 = 2 a x moves the peak to xi = +2 a."""
    degree, a = 3, 0.375
    coef = np.zeros((2, len(ort.zernike_terms(degree))))
    coef[1, ort.zernike_terms(degree).index((1, 1))] = a
    for centre, check in (([[0.0, 0.0], [2 * a, 0.0]], lambda s: abs(s[0] - 1.0) <= 1e-12 and abs(s[1] - 1.0) <= 1e-12),
                          ([[0.0, 0.0], [-2 * a, 0.0]], lambda s: s[1] < 0.5)):
        psf, strehl = hip_engine.psf(coef, degree, 64, 32, 0.125, centre=np.array(centre))
        assert check(strehl), (centre, strehl)
    pe, se = hip_engine.psf(coef[1:], degree, 64, 32, 0.125, centre=np.array([[-2 * a, 0.0]]))
    p1, s1 = ort.psf(coef[1], degree, npupil=64, nimg=32, dxi=0.125, centre=(-2 * a, 0.0), engine=hip_engine)
    assert np.array_equal(p1, pe[0]) and s1 == se[0] == strehl[1]


@pytest.mark.parametrize("kw", (dict(degree=0), dict(degree=11), dict(npupil=16), dict(npupil=40), dict(npupil=1040), dict(nimg=0),
                                dict(nimg=24), dict(nimg=144), dict(dxi=0.0), dict(dxi=-0.1)))
def test_bad_arguments(hip_engine, kw):
    args = dict(degree=4, npupil=32, nimg=16, dxi=0.125)
    args.update(kw)
    with pytest.raises(_capi.OrtError) as e:
        hip_engine.psf(np.zeros((1, max(args["degree"], 1) * (max(args["degree"], 1) + 3) // 2)), **args)
    assert e.value.code == -1                                         # ORT_EINVAL
    if kw == dict(degree=0):                                          # and the two required pointers
        z = np.zeros(14)
        for coef, strehl in ((None, z.ctypes.data), (z.ctypes.data, None)):
            assert hip_engine.ctx.lib.ort_psf_f64(hip_engine.ctx.h, 1, 4, coef, None, 32, 16, 0.125, None, None, strehl, 0) == -1
