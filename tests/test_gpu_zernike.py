"""`ort_zernike_fit_f64`: the Zernike wavefront fit of full_trace results on the device (the workflow of the reference's
misc/Zernike_fit.jl: wavegrad -> fit of the Zernike gradients) against `np.linalg.lstsq` on a design matrix built from the
explicit factorial formula of R_n^m and the polar chain rule — no code shared with the kernel's recurrences."""
from math import factorial, sqrt

import numpy as np
import pytest

import opticalraytracing_jl_amd as ort
from opticalraytracing_jl_amd import _capi
from tests import common as cm

pytestmark = pytest.mark.gpu
LAM = 587.5618e-6


def reference_G(rho, theta, degree):
    """[2 N][nterms]: rows dZ_j/dx, dZ_j/dy per ray, j in OSA/ANSI order without piston, Zernike.jl's orthonormal convention.
    A ray at rho = 0 takes the limit: only |m| = 1 contributes, with slope N R'(0) along x (m = 1) or y (m = -1)."""
    rho, theta = np.asarray(rho, dtype=np.float64), np.asarray(theta, dtype=np.float64)
    terms = [(n, m) for n in range(1, degree + 1) for m in range(-n, n + 1, 2)]
    G = np.zeros((2 * rho.size, len(terms)))
    c, s, zero = np.cos(theta), np.sin(theta), rho == 0
    rs = np.where(zero, 1.0, rho)
    for j, (n, m) in enumerate(terms):
        mu, N = abs(m), sqrt(2 * (n + 1) / (2 if m == 0 else 1))
        R, dR = np.zeros_like(rho), np.zeros_like(rho)
        for k in range((n - mu) // 2 + 1):
            a = (-1) ** k * factorial(n - k) / (factorial(k) * factorial((n + mu) // 2 - k) * factorial((n - mu) // 2 - k))
            R += a * rho ** (n - 2 * k)
            if n - 2 * k > 0:
                dR += a * (n - 2 * k) * rho ** (n - 2 * k - 1)
        ang, dang = (np.cos(mu * theta), -mu * np.sin(mu * theta)) if m >= 0 else (np.sin(mu * theta), mu * np.cos(mu * theta))
        zr, zt = N * dR * ang, N * R * dang / rs                       # dZ/drho, (1 / rho) dZ/dtheta
        G[0::2, j] = np.where(zero, N * dR if m == 1 else 0.0, zr * c - zt * s)
        G[1::2, j] = np.where(zero, N * dR if m == -1 else 0.0, zr * s + zt * c)
    return G


def lstsq_fit(ex, ey, rho, theta, nu, degree):
    G = reference_G(rho, theta, degree)
    b = np.empty(2 * len(ex))
    b[0::2], b[1::2] = ex * nu / LAM, ey * nu / LAM
    c = np.linalg.lstsq(G, b, rcond=None)[0]
    return c, sqrt(np.mean((G @ c - b) ** 2))


@pytest.mark.parametrize("degree", (1, 4, 5, 7, 9, 10))
def test_fit_matches_lstsq(hip_engine, degree):
    """nterms + 1 = 3, 15, 21, 36, 55, 66: every tile count 1..5, either side of the 16-column boundaries.  Three slabs of
    cap 700 with 697 (no multiple of a k-step or a slab), 130 and 0 valid entries; one ray at exactly rho = 0."""
    import torch
    rng = np.random.default_rng(20260 + degree)
    nb, cap, counts, nu = 3, 700, np.array([697, 130, 0], dtype=np.int64), np.array([-0.2, -0.17, -0.19])
    nterms = len(ort.zernike_terms(degree))
    rho, theta = np.sqrt(rng.uniform(size=(nb, cap))), rng.uniform(-np.pi, np.pi, size=(nb, cap))
    rho[0, 5] = 0.0
    ex, ey, want = np.zeros((nb, cap)), np.zeros((nb, cap)), []
    for b in range(2):
        m = counts[b]
        g = reference_G(rho[b, :m], theta[b, :m], degree) @ rng.normal(size=nterms) + 1e-3 * rng.normal(size=2 * m)
        ex[b, :m], ey[b, :m] = g[0::2] * LAM / nu[b], g[1::2] * LAM / nu[b]
        want.append(lstsq_fit(ex[b, :m], ey[b, :m], rho[b, :m], theta[b, :m], nu[b], degree))
    coef, resid, info = hip_engine.zernike_fit(ex, ey, rho, theta, counts, nu, LAM, degree)
    worst = 0.0
    for b, (c_ref, r_ref) in enumerate(want):
        dev = np.abs(coef[b] - c_ref).max() / max(1.0, np.abs(c_ref).max())
        worst = max(worst, dev)
        print(f"degree {degree} slab {b}: coefficient deviation {dev:.3e}, resid {resid[b]:.12e} (lstsq {r_ref:.12e})")
        assert dev <= 1e-11
        assert abs(resid[b] - r_ref) <= 1e-9 * r_ref
    cm.report(f"zernike_fit degree {degree}: worst coefficient deviation from lstsq {worst:.2e} (bound 1e-11)")
    assert info[0] == 0 and info[1] == 0 and info[2] != 0
    assert np.isnan(coef[2]).all() and np.isnan(resid[2])
    dv = torch.device("cuda:0")
    d = [torch.from_numpy(a).to(dv) for a in (ex, ey, rho, theta, counts, nu)]
    torch.cuda.synchronize(dv)
    runs = [hip_engine.zernike_fit(d[0], d[1], d[2], d[3], d[4], d[5], LAM, degree) for _ in range(2)]
    hip_engine.ctx.synchronize()
    for dc, dr, di in runs:                                           # device pointers == host pointers, and run to run
        assert np.array_equal(dc.cpu().numpy(), coef, equal_nan=True) and np.array_equal(dr.cpu().numpy(), resid, equal_nan=True)
        assert np.array_equal(di.cpu().numpy(), info)


@pytest.mark.parametrize("H", (0.0, 1.0))
def test_fit_of_a_real_full_trace(hip_engine, H):
    """The reference's Tessar, k_rays = 16, degree 6: device-resident full_trace vectors fitted where they lie."""
    import torch
    k, degree = 16, 6
    system = ort.solve(cm.tessar(), cm.TESSAR_A, cm.TESSAR_H, engine=hip_engine)
    aim = ort.full_trace_aim(system.layout, system, H, engine=hip_engine)
    pres = ort.extended_prescription(system.layout, aim.focus)
    axes = np.concatenate([ort.linrange(aim.y1, aim.y2, k), ort.linrange(0.0, aim.y_EP, k // 2)])
    bundle = dict(system=0, stop=aim.stop, U=aim.U, V=0.0, a_stop=aim.a_stop, hprime=aim.hprime, yaxis_off=0, xaxis_off=k)
    dv, cap = torch.device("cuda:0"), 2 * k * (k // 2)
    d_axes = torch.from_numpy(axes).to(dv)
    ex, ey, rho, th = (torch.zeros((1, cap), dtype=torch.float64, device=dv) for _ in range(4))
    cnt = torch.zeros(1, dtype=torch.int64, device=dv); rms = torch.zeros(1, dtype=torch.float64, device=dv)
    nu = torch.full((1,), aim.nu, dtype=torch.float64, device=dv)
    sysd = hip_engine.system(pres)
    torch.cuda.synchronize(dv)
    _capi.check(hip_engine.ctx.lib.ort_full_trace_f64(hip_engine.ctx.h, sysd.h, 1, _capi.make_bundles([bundle]), d_axes.data_ptr(), axes.size,
                                                      k, k // 2, ex.data_ptr(), ey.data_ptr(), rho.data_ptr(), th.data_ptr(),
                                                      cnt.data_ptr(), rms.data_ptr(), _capi.ORT_DEVICE_PTRS))
    coef, resid, info = hip_engine.zernike_fit(ex, ey, rho, th, cnt, nu, LAM, degree)
    hip_engine.ctx.synchronize()
    m = int(cnt[0])
    assert m >= 64 and int(info[0]) == 0
    c_ref, r_ref = lstsq_fit(*(t[0, :m].cpu().numpy() for t in (ex, ey, rho, th)), aim.nu, degree)
    dev = np.abs(coef[0].cpu().numpy() - c_ref).max() / max(1.0, np.abs(c_ref).max())
    print(f"Tessar H = {H}: {m} entries, coefficient deviation {dev:.3e}, resid {float(resid[0]):.6e} waves (lstsq {r_ref:.6e})")
    assert dev <= 1e-11
    err = ort.RealRayError(*(t[0, :m].cpu().numpy() for t in (ex, ey)), aim.nu, rho[0, :m].cpu().numpy(), th[0, :m].cpu().numpy(), H, float(rms[0]))
    c_api, _, i_api = ort.zernike_fit(err, degree, engine=hip_engine)    # the public entry on a host-resident RealRayError
    assert i_api == 0 and np.abs(c_api - c_ref).max() <= 1e-11 * max(1.0, np.abs(c_ref).max())


def test_bad_arguments(hip_engine):
    z = np.zeros((1, 64))
    for degree, lam in ((0, LAM), (11, LAM), (4, 0.0)):
        with pytest.raises(_capi.OrtError) as e:
            hip_engine.zernike_fit(z, z, z, z, np.array([64]), np.array([-0.2]), lam, degree)
        assert e.value.code == -1                                     # ORT_EINVAL
