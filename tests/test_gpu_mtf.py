"""`ort_mtf_f64`: tangential and sagittal OTF / MTF of Zernike wavefronts on the device, against the shifted products of the
pupil field summed by numpy in complex128 — W from the explicit factorial formula of R_n^m.  No code shared with the kernel's
recurrences and no Gram matrix.  Bound 1e-11 absolute on values of modulus <= 1, the PSF's bound on the PSF's argument: the
float64 reference lies within 3.6e-15 of the same sums in long double; the kernel's recurrences hold 1e-14 relative on
|W| <= 10 waves, a coherent phase error of at most 2 pi 1e-13."""
from math import factorial, sqrt

import numpy as np
import pytest

import opticalraytracing_jl_amd as ort
from opticalraytracing_jl_amd import _capi
from tests import common as cm

pytestmark = pytest.mark.gpu
TOL = 1e-11


def reference_otf(coef, degree, npupil):
    """[nb][2][npupil] complex from coef [nb][nterms]: the definition in include/ort.h, shear by shear."""
    x = (2.0 * np.arange(npupil) + 1.0 - npupil) / npupil
    X, Y = np.meshgrid(x, x)                                          # X[j][k] = x_k, Y[j][k] = y_j
    mask, rho, theta = X * X + Y * Y <= 1.0, np.hypot(X, Y), np.arctan2(Y, X)
    Z = []
    for n, m in ort.zernike_terms(degree):
        mu, R = abs(m), np.zeros_like(rho)
        for k in range((n - mu) // 2 + 1):
            R += (-1) ** k * factorial(n - k) / (factorial(k) * factorial((n + mu) // 2 - k) * factorial((n - mu) // 2 - k)) * rho ** (n - 2 * k)
        Z.append(sqrt(2 * (n + 1) / (2 if m == 0 else 1)) * R * (np.cos(mu * theta) if m >= 0 else np.sin(mu * theta)))
    P = mask * np.exp(2j * np.pi * np.tensordot(np.asarray(coef, dtype=np.float64), np.array(Z), axes=1))
    H = np.empty((len(P), 2, npupil), dtype=np.complex128)
    for d in range(npupil):
        H[:, 0, d] = (P[:, :, d:] * np.conj(P[:, :, :npupil - d])).sum(axis=(1, 2))
        H[:, 1, d] = (P[:, d:, :] * np.conj(P[:, :npupil - d, :])).sum(axis=(1, 2))
    return H / mask.sum()


def wavefronts(rng, nb, degree, rms):
    """Random coefficient rows scaled to the given wavefront RMS in waves (the terms are orthonormal)."""
    c = rng.normal(size=(nb, len(ort.zernike_terms(degree))))
    return c / np.linalg.norm(c, axis=1, keepdims=True) * np.reshape(rms, (-1, 1))


@pytest.mark.parametrize("npupil,degree", ((32, 1), (48, 10), (80, 7), (256, 10), (272, 6)))
def test_mtf_matches_direct_autocorrelation(hip_engine, npupil, degree):
    """Two block diagonals; an odd block count; 80 = 5 row panels, cut into spans and folded at three bundles; several
    diagonals per wave (16 of them, one group); and 272, the smallest npupil whose 17 block diagonals are split over two
    groups of workgroups.  1024 runs the same instantiation as 272 (four diagonals per wave) with five groups, so it is no
    case of its own.  Bundle 2 has no fit."""
    import torch
    rng = np.random.default_rng(47000 + npupil + degree)
    info = np.array([0, 0, 1], dtype=np.int32)
    coef = wavefronts(rng, 3, degree, [0.1, 1.0, 3.0])
    coef[2] = np.nan
    want = reference_otf(coef[:2], degree, npupil)
    mtf, otf = hip_engine.mtf(coef, degree, npupil, info=info, want_otf=True)
    dev = max(np.abs(otf[:2] - want).max(), np.abs(mtf[:2] - np.abs(want)).max())
    print(f"mtf ({npupil}, {degree}): worst deviation {dev:.3e}, H(0) - 1 = {abs(otf[0, 0, 0] - 1):.1e}")
    cm.report(f"mtf npupil {npupil} degree {degree}: worst deviation from the direct autocorrelation {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL
    assert np.array_equal(mtf[:2], np.hypot(otf[:2].real, otf[:2].imag))
    assert np.isnan(mtf[2]).all() and np.isnan(otf[2].real).all() and np.isnan(otf[2].imag).all()
    only, none = hip_engine.mtf(coef, degree, npupil, info=info)
    assert none is None and np.array_equal(only, mtf, equal_nan=True)
    dv = torch.device("cuda:0")
    d = [torch.from_numpy(a).to(dv) for a in (coef, info)]
    torch.cuda.synchronize(dv)
    runs = [hip_engine.mtf(d[0], degree, npupil, info=d[1], want_otf=True) for _ in range(2)]
    hip_engine.ctx.synchronize()
    for dm, do in runs:                                               # device pointers == host pointers, and run to run
        assert np.array_equal(dm.cpu().numpy(), mtf, equal_nan=True)
        assert np.array_equal(torch.view_as_real(do).cpu().numpy(), np.stack((otf.real, otf.imag), axis=-1), equal_nan=True)


def test_many_bundles_route(hip_engine):
    """1200 bundles x 2 axes exceed four workgroups per compute unit: one workgroup per curve, written without a workspace.
    Every bundle has its own coefficients, so a slot or axis mix-up between bundles fails."""
    rng = np.random.default_rng(27182)
    nb, npupil, degree = 1200, 32, 4
    coef = wavefronts(rng, nb, degree, rng.uniform(0.05, 1.0, size=nb))
    want = reference_otf(coef, degree, npupil)
    mtf, otf = hip_engine.mtf(coef, degree, npupil, want_otf=True)
    dev = max(np.abs(otf - want).max(), np.abs(mtf - np.abs(want)).max())
    cm.report(f"mtf, 1200 bundles: worst deviation from the direct autocorrelation {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL
    assert np.array_equal(mtf, np.hypot(otf.real, otf.imag))


def test_conventions(hip_engine):
    """Normalisation, sign, frequency unit and axis naming, independently of the reference function.  In the tilt case Im H_1
    is checked against the bound, not against exact zero: s c - c s cancels only to rounding when the two products are
    accumulated into one tile by two matrix instructions, which is how Im is formed (no third accumulator tile)."""
    degree, npupil, a = 3, 64, 0.375
    terms = ort.zernike_terms(degree)
    coef = np.zeros((3, len(terms)))
    coef[1, terms.index((1, 1))] = a
    coef[2, terms.index((2, -2))] = 0.8
    mtf, otf = hip_engine.mtf(coef, degree, npupil, want_otf=True)
    d = np.arange(npupil)
    assert abs(otf[0, 0, 0] - 1.0) <= 1e-12 and np.all(otf[0].imag == 0.0)       # flat wavefront
    assert np.array_equal(otf[0, 0].real, otf[0, 1].real) and np.array_equal(mtf[0, 0], mtf[0, 1])
    assert np.all(np.diff(mtf[0, 0]) <= 0.0)
    sel = mtf[1, 0] > 0.01                                                        # tilt 2 a x: phase +2 pi 2 a 2 d / npupil
    assert sel.sum() > npupil // 2
    assert np.abs(np.angle(otf[1, 0] * np.exp(-2j * np.pi * 2 * a * 2 * d / npupil)))[sel].max() <= 1e-11
    assert np.abs(otf[1, 1].imag).max() <= TOL and np.abs(otf[1, 1].real - otf[0, 1].real).max() <= TOL
    assert np.abs(otf[2, 0] - otf[2, 1]).max() <= TOL and np.ptp(mtf[2, 0] - mtf[0, 0]) > 0.1      # Z_2^-2 is symmetric in x <-> y
    freq, sag, tan = ort.mtf(coef[2], degree, npupil=npupil, engine=hip_engine)
    assert np.array_equal(freq, ort.mtf_frequencies(npupil)) and np.array_equal(freq, 2.0 * d / npupil)
    assert np.array_equal(sag, mtf[2, 0]) and np.array_equal(tan, mtf[2, 1])


@pytest.mark.parametrize("kw", (dict(degree=0), dict(degree=11), dict(npupil=16), dict(npupil=40), dict(npupil=1040)))
def test_bad_arguments(hip_engine, kw):
    args = dict(degree=4, npupil=32)
    args.update(kw)
    with pytest.raises(_capi.OrtError) as e:
        hip_engine.mtf(np.zeros((1, max(args["degree"], 1) * (max(args["degree"], 1) + 3) // 2)), **args)
    assert e.value.code == -1                                         # ORT_EINVAL
    if kw == dict(degree=0):                                          # NULL coef, and both outputs NULL
        z = np.zeros(128)
        for coef, mtf in ((None, z.ctypes.data), (z.ctypes.data, None)):
            assert hip_engine.ctx.lib.ort_mtf_f64(hip_engine.ctx.h, 1, 4, coef, None, 32, None, mtf, 0) == -1
