"""`ort_spot_radii_f64` / `_f32`: centroid, encircled-energy and GEO radii of full_trace slabs on the device, against the
definition in numpy: mu with math.fsum (exact), q in float64, np.partition.  Nothing shared with the kernel's radix selection.

Bound 1e-12 x max(|ex|, |ey|) absolute on radii and centroid: an order statistic moves by at most |delta mu| when the centroid
moves; the device's tree sums hold mu to about (log2 n + a few) eps, <~ 3e-15 of the scale for n <= 2^20; q and sqrt add a few
eps.  1e-12 is the project's bar for the merged-moment RMS and leaves more than 100 x margin."""
import math

import numpy as np
import pytest

import opticalraytracing_jl_amd as ort
from opticalraytracing_jl_amd import _capi
from tests import common as cm

pytestmark = pytest.mark.gpu
TOL = 1e-12


def reference(ex, ey, counts, fractions):
    """(centroid [nb][2], radii [nb][nfrac]) by the definition in include/ort.h; NaN rows for empty bundles."""
    cen, rad = np.full((len(counts), 2), np.nan), np.full((len(counts), len(fractions)), np.nan)
    for b, n in enumerate(counts):
        if n > 0:
            x, y = ex[b, :n].astype(np.float64), ey[b, :n].astype(np.float64)
            cen[b] = math.fsum(x.tolist()) / n, math.fsum(y.tolist()) / n
            q = (x - cen[b, 0]) ** 2 + (y - cen[b, 1]) ** 2
            ks = [min(n, max(1, math.ceil(f * n))) for f in fractions]
            rad[b] = np.sqrt(np.partition(q, [k - 1 for k in ks])[[k - 1 for k in ks]])
    return cen, rad


def spots(seed, counts, dtype):
    """Anisotropic normal spots with a non-zero mean, one per bundle; every slab's tail beyond its count is NaN."""
    rng = np.random.default_rng(seed)
    cap = max(max(counts), 1)
    ex, ey = (np.full((len(counts), cap), np.nan, dtype=dtype) for _ in range(2))
    for b, n in enumerate(counts):
        ex[b, :n] = rng.normal(0.3 + 0.01 * (b % 7), 0.02, n)
        ey[b, :n] = rng.normal(-0.1, 0.005 * (1 + b % 3), n)
    return ex, ey


FOUR = (0.5, 0.8, 0.9, 1.0)
LISTS = ((0, 1, 2, 255, 256, 257, 4097), (16383, 16384, 16385), (8192 * 3 + 5,), (8193, 16384))
CASES = [(c, t, f) for c in LISTS for t in (np.float64, np.float32) for f in (FOUR, (1 / 3,))]
CASES += [((300,) * 1200, np.float64, FOUR), ((16385,) * 1100, np.float32, FOUR)]


@pytest.mark.parametrize("counts,dtype,fractions", CASES,
                         ids=[f"{len(c)}x{c[-1]}-{np.dtype(t).name}-{len(f)}" for c, t, f in CASES])
def test_radii_match_the_definition(hip_engine, counts, dtype, fractions):
    """Around the workgroup size with an empty bundle, in LDS (cap 4097); the LDS-route edge, where a slab of 16385 leaves
    the LDS route and the bundle of 16384 ends exactly on a span edge (three spans); four spans, the last of 5 entries; the
    largest slab the LDS route takes (cap 16384: 128 KB of q, two chunks); 1200 bundles in LDS, one workgroup each; 1100
    bundles of 16385 entries, one workgroup each, q recomputed in every pass."""
    import torch
    ex, ey = spots(7000 + len(counts) + len(fractions), counts, dtype)
    scale = max(np.nanmax(np.abs(ex)), np.nanmax(np.abs(ey)))
    want_c, want_r = reference(ex, ey, counts, fractions)
    cen, rad = hip_engine.spot_radii(ex, ey, counts, fractions)
    live = np.asarray(counts) > 0
    dev = max(np.abs(cen[live] - want_c[live]).max(), np.abs(rad[live] - want_r[live]).max()) / scale
    cm.report(f"spot_radii {len(counts)} x {counts[-1]} {np.dtype(dtype).name}, {len(fractions)} fractions: worst deviation from "
              f"fsum / partition {dev:.2e} of the scale (bound {TOL:g})")
    assert dev <= TOL
    assert np.isnan(cen[~live]).all() and np.isnan(rad[~live]).all()
    dv = torch.device("cuda:0")
    d = [torch.from_numpy(a).to(dv) for a in (ex, ey, np.asarray(counts, dtype=np.int64))]
    torch.cuda.synchronize(dv)
    runs = [hip_engine.spot_radii(d[0], d[1], d[2], fractions) for _ in range(2)]
    hip_engine.ctx.synchronize()
    for dc, dr in runs:                                               # device pointers == host pointers, and run to run
        assert np.array_equal(dc.cpu().numpy(), cen, equal_nan=True) and np.array_equal(dr.cpu().numpy(), rad, equal_nan=True)


@pytest.mark.parametrize("n", (4096, 40000))
def test_exact_selection_under_ties(hip_engine, n):
    """Small integers, point-symmetric: every partial sum is exact, mu is exactly 0 and q holds a few dozen distinct integers
    with thousands of ties.  4096 in LDS, 40000 in one bundle cut into spans.  f n is an integer for 0.25, 0.5, 0.75, 1."""
    rng = np.random.default_rng(n)
    half = rng.integers(-8, 9, size=(2, n // 2)).astype(np.float64)
    ex, ey = np.concatenate([half, -half], axis=1)[:, None, :]
    fractions = (1e-9, 0.25, 1 / 3, 0.5, 0.61, 0.75, 0.999, 1.0)
    cen, rad = hip_engine.spot_radii(ex, ey, [n], fractions)
    q_sorted = np.sort(ex[0] ** 2 + ey[0] ** 2)
    ks = np.array([min(n, max(1, math.ceil(f * n))) for f in fractions])
    assert np.array_equal(cen, np.zeros((1, 2)))
    assert np.array_equal(np.rint(rad[0] ** 2), q_sorted[ks - 1])


def test_through_the_public_interface(hip_engine):
    """full_trace of the reference's Tessar at k_rays = 64, then the radii of the returned vectors."""
    system = ort.solve(cm.tessar(), cm.TESSAR_A, cm.TESSAR_H, engine=hip_engine)
    err = ort.full_trace(system, 1.0, 64, engine=hip_engine)
    fractions = (0.5, 0.8, 1.0)
    cen, rad = ort.spot_radii(err, engine=hip_engine)
    scale = max(np.abs(err.x).max(), np.abs(err.y).max())
    mux, muy = math.fsum(err.x.tolist()) / len(err.x), math.fsum(err.y.tolist()) / len(err.y)
    assert abs(rad[-1] - np.hypot(err.x - mux, err.y - muy).max()) <= TOL * scale
    assert abs(cen[0] - mux) <= TOL * scale and abs(cen[1] - muy) <= TOL * scale
    assert np.all(np.diff(rad) >= 0.0) and rad[0] > 0.0
    c2, r2 = hip_engine.spot_radii(err.x[None], err.y[None], [len(err.x)], fractions)
    assert np.array_equal(c2[0], cen) and np.array_equal(r2[0], rad)


@pytest.mark.parametrize("fractions", ((), (0.1,) * 9, (0.5, 0.0), (1.5,), (0.5, float("nan"))))
def test_bad_arguments(hip_engine, fractions):
    z = np.zeros((1, 8))
    with pytest.raises(_capi.OrtError) as e:
        hip_engine.spot_radii(z, z, [8], fractions)
    assert e.value.code == -1                                         # ORT_EINVAL
    if not fractions:                                                 # a NULL among the required pointers; cap < 1; nb < 0
        lib, h, p = hip_engine.ctx.lib, hip_engine.ctx.h, z.ctypes.data
        count, half = np.array([8], dtype=np.int64), np.array([0.5])
        cnt, f = count.ctypes.data, half.ctypes.data
        good = [h, 1, 8, cnt, p, p, 1, f, None, p, 0]
        for i in (3, 4, 5, 7, 9):
            assert lib.ort_spot_radii_f64(*(None if j == i else v for j, v in enumerate(good))) == -1
        assert lib.ort_spot_radii_f32(h, 1, 0, cnt, p, p, 1, f, None, p, 0) == -1
        assert lib.ort_spot_radii_f64(h, -1, 8, cnt, p, p, 1, f, None, p, 0) == -1
