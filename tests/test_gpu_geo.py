"""`ort_geo_mtf_f64` / `_f32` and `ort_spot_image_f64` / `_f32`: geometric MTF and spot density of full_trace slabs on the device,
against their definitions in numpy.  Nothing shared with the kernels' seed-and-rotate recurrence or their histograms.

MTF bound 1e-12 absolute on otf, the bar of the spot chain (test_gpu_spot_radii.py): |nu d| stays below about 80 cycles here, so
the phase is conditioned to 2 pi 80 eps ~ 1e-13, 10 x inside it (worst measured over these cases: 1.3e-14; the 24,581-entry
bundle: 5.6e-16).  The reference forms nu_m d in long double and reduces it by rint there; the reduced phase, |p| <= 1/2, then goes
to float64 (an error of at most 2 pi 2^-54 ~ 3.5e-16 per term) so that cos / sin of 25 M terms take a fraction of a second.
The spot image is integer counting: compared with np.array_equal."""
import numpy as np
import pytest

import opticalraytracing_jl_amd as ort
from opticalraytracing_jl_amd import _capi
from opticalraytracing_jl_amd.api import LAMBDA
from tests import common as cm
from tests.test_gpu_spot_radii import spots                          # the input maker of the spot chain's tests

pytestmark = pytest.mark.gpu
TOL = 1e-12


def reference(ex, ey, counts, scale, centre, nfreq=None, dnu=None, nimg=None, dxi=None):
    """nfreq given: otf [nb][2][nfreq] complex by the definition, NaN rows for empty bundles.  nimg given: (image, lsf, outside)
    by the three operations per coordinate and np.add.at.  d is formed in float64 as include/ort.h does: one product, one
    difference."""
    nb = len(counts)
    frame = [(b, n, ex[b, :n].astype(np.float64) * (1.0 if scale is None else scale[b]) - (0.0 if centre is None else centre[b, 0]),
              ey[b, :n].astype(np.float64) * (1.0 if scale is None else scale[b]) - (0.0 if centre is None else centre[b, 1]))
             for b, n in enumerate(counts)]
    if nfreq is not None:
        H, nu = np.full((nb, 2, nfreq), np.nan + 0j), (np.arange(nfreq) * dnu).astype(np.longdouble)[:, None]
        for b, n, dx, dy in frame:
            for axis, d in enumerate((dx, dy)):
                for m0 in range(0, nfreq if n else 0, 64):
                    p = nu[m0:m0 + 64] * d.astype(np.longdouble)
                    p = 2.0 * np.pi * (p - np.rint(p)).astype(np.float64)
                    H[b, axis, m0:m0 + 64] = np.cos(p).mean(axis=1) + 1j * np.sin(p).mean(axis=1)
        return H
    image, lsf, outside = np.zeros((nb, nimg, nimg), np.int32), np.zeros((nb, 2, nimg), np.int32), np.zeros(nb, np.int64)
    for b, n, dx, dy in frame:
        ix, iy = (np.floor(d / dxi + 0.5).astype(np.int64) + nimg // 2 for d in (dx, dy))
        okx, oky = (ix >= 0) & (ix < nimg), (iy >= 0) & (iy < nimg)
        np.add.at(image[b], (iy[okx & oky], ix[okx & oky]), 1)
        np.add.at(lsf[b, 0], ix[okx], 1)
        np.add.at(lsf[b, 1], iy[oky], 1)
        outside[b] = n - (okx & oky).sum()
    return image, lsf, outside


def inputs(seed, counts, dtype, scale, centre):
    """(ex, ey, count, scale [nb] or None, centre [nb][2] or None) on the host and the same as CUDA tensors: the anisotropic
    normal spots of test_gpu_spot_radii.py, mean (0.3 .. 0.36, -0.1), NaN beyond count."""
    import torch
    nb = len(counts)
    host = spots(seed, counts, dtype) + (np.asarray(counts, dtype=np.int64), None if scale is None else np.full(nb, scale),
                                         None if centre is None else np.tile(np.float64(centre), (nb, 1)))
    dev = [None if a is None else torch.from_numpy(a).to("cuda:0") for a in host]
    torch.cuda.synchronize()
    return host, dev


LISTS = ((0, 1, 2, 255, 256, 257, 4097), (8192 * 3 + 5,))
MANY = (300,) * 1200
FRAMES = ((None, (0.3, -0.1)), (0.5, None))                          # (scale, centre): each NULL once, each given once
MTF_CASES = [(c, f, t, k) for c in LISTS for f in (1, 16, 17, 512) for t in (np.float64, np.float32) for k in (0, 1)]
MTF_CASES += [(MANY, 33, np.float64, 0), (MANY, 33, np.float32, 1)]


@pytest.mark.parametrize("counts,nfreq,dtype,k", MTF_CASES,
                         ids=[f"{len(c)}x{c[-1]}-{f}-{np.dtype(t).name}-frame{k}" for c, f, t, k in MTF_CASES])
def test_geo_mtf_matches_the_definition(hip_engine, counts, nfreq, dtype, k):
    """Around the workgroup size with an empty bundle (five spans of one chunk); 25 spans, the last of 5 entries; 1200 bundles,
    one workgroup each.  nfreq 1 and 16: one block cut over four waves; 17: two blocks, the second of one sample; 512: 64
    (axis, block) units, eight per wave.  dnu = 0.5: up to 77 cycles of phase."""
    import torch
    (ex, ey, cnt, scale, centre), d = inputs(9000 + len(counts) + nfreq, counts, dtype, *FRAMES[k])
    want = reference(ex, ey, counts, scale, centre, nfreq=nfreq, dnu=0.5)
    mtf, otf = hip_engine.geo_mtf(ex, ey, cnt, nfreq, 0.5, scale=scale, centre=centre, want_otf=True)
    live = np.asarray(counts) > 0
    dev = np.abs(otf[live] - want[live]).max()
    cm.report(f"geo_mtf {len(counts)} x {counts[-1]} nfreq {nfreq} {np.dtype(dtype).name} frame {k}: worst deviation from the "
              f"definition {dev:.2e} (bound {TOL:g})")
    assert dev <= TOL
    assert np.array_equal(mtf[live], np.hypot(otf[live].real, otf[live].imag)) and np.all(otf[live][:, :, 0] == 1.0)
    assert np.isnan(mtf[~live]).all() and np.isnan(otf[~live].real).all() and np.isnan(otf[~live].imag).all()
    only, none = hip_engine.geo_mtf(ex, ey, cnt, nfreq, 0.5, scale=scale, centre=centre)
    assert none is None and np.array_equal(only, mtf, equal_nan=True)
    runs = [hip_engine.geo_mtf(d[0], d[1], d[2], nfreq, 0.5, scale=d[3], centre=d[4], want_otf=True) for _ in range(2)]
    hip_engine.ctx.synchronize()
    for dm, do in runs:                                               # device pointers == host pointers, and run to run
        assert np.array_equal(dm.cpu().numpy(), mtf, equal_nan=True)
        assert np.array_equal(torch.view_as_real(do).cpu().numpy(), np.stack((otf.real, otf.imag), axis=-1), equal_nan=True)


def test_conventions(hip_engine):
    """Sign and frequency unit: a spot wholly at (xi0, eta0) gives exp(+i 2 pi nu xi0) on axis 0 and the same with eta0 on
    axis 1.  A mirror-symmetric spot has a real H_0.  H(0) is exactly 1."""
    xi0, eta0, nu = 0.37, -0.21, 0.25 * np.arange(64)
    _, otf = hip_engine.geo_mtf(np.array([[xi0]]), np.array([[eta0]]), [1], 64, 0.25, want_otf=True)
    assert np.abs(otf[0, 0] - np.exp(2j * np.pi * nu * xi0)).max() <= TOL
    assert np.abs(otf[0, 1] - np.exp(2j * np.pi * nu * eta0)).max() <= TOL
    h = np.random.default_rng(5).normal(0.0, 0.05, 5000)
    x = np.concatenate([h, -h])[None]
    mtf, otf = hip_engine.geo_mtf(x, 0.5 * x, [x.size], 64, 0.25, want_otf=True)
    assert np.abs(otf[0, 0].imag).max() <= TOL and np.all(otf[0, :, 0] == 1.0) and np.all(mtf[0, :, 0] == 1.0)
    assert mtf[0, 0, 1:].max() < 1.0 and np.all(mtf[0, 1, 1:8] > mtf[0, 0, 1:8])       # the narrower axis keeps more contrast


IMG_CASES = [(c, t, n) for c in LISTS + (MANY,) for t in (np.float64, np.float32) for n in (16, 128)]


@pytest.mark.parametrize("counts,dtype,nimg", IMG_CASES, ids=[f"{len(c)}x{c[-1]}-{np.dtype(t).name}-{n}" for c, t, n in IMG_CASES])
def test_spot_image_is_exact(hip_engine, counts, dtype, nimg):
    """The same lists: spans with global atomics (7 and 1 bundles) and one workgroup per bundle (1200).  The image spans
    +-0.02 about the first bundle's mean, one sigma_x at scale 1 and two at scale 0.5 (centre scaled alike): entries fall
    outside in x, few in y.  nimg 128 takes 65 KB of LDS."""
    frame = (0.5, (0.15, -0.05)) if dtype == np.float32 else FRAMES[0]
    (ex, ey, cnt, scale, centre), d = inputs(9100 + len(counts) + nimg, counts, dtype, *frame)
    dxi = 0.04 / nimg
    want = reference(ex, ey, counts, scale, centre, nimg=nimg, dxi=dxi)
    got = hip_engine.spot_image(ex, ey, cnt, nimg, dxi, scale=scale, centre=centre)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    image, lsf, outside = got
    assert np.array_equal(image.sum(axis=(1, 2)) + outside, counts) and outside.sum() > 0
    assert np.all(lsf[:, 0] >= image.sum(axis=1)) and np.all(lsf[:, 1] >= image.sum(axis=2))
    empty = np.asarray(counts) == 0
    assert not image[empty].any() and not lsf[empty].any() and not outside[empty].any()
    runs = [hip_engine.spot_image(d[0], d[1], d[2], nimg, dxi, scale=d[3], centre=d[4]) for _ in range(2)]
    hip_engine.ctx.synchronize()
    for run in runs:
        assert all(np.array_equal(r.cpu().numpy(), g) for r, g in zip(run, got))


@pytest.mark.parametrize("case", ("ties", "one_bin"))
def test_spot_image_ties(hip_engine, case):
    """40,000 entries on the integers -8 .. 8 with dxi = 1 and no centre: every entry on a bin centre, thousands per bin, the
    value 8 outside, one bundle cut into five spans.  And a spot wholly in one bin: every wave adds its count with one atomic."""
    n = 40000
    if case == "ties":
        ex, ey = np.random.default_rng(n).integers(-8, 9, size=(2, 1, n)).astype(np.float64)
    else:
        ex, ey = np.full((1, n), 3.2), np.full((1, n), -1.4)
    want = reference(ex, ey, [n], None, None, nimg=16, dxi=1.0)
    got = hip_engine.spot_image(ex, ey, [n], 16, 1.0)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    if case == "one_bin":
        assert got[0][0, 7, 11] == n and got[1][0, 0, 11] == n and got[1][0, 1, 7] == n and got[2][0] == 0


def test_through_the_public_interface(hip_engine):
    """full_trace of the reference's Tessar at k_rays = 64, then both analyses of the returned vectors."""
    system = ort.solve(cm.tessar(), cm.TESSAR_A, cm.TESSAR_H, engine=hip_engine)
    err = ort.full_trace(system, 1.0, 64, engine=hip_engine)
    x, y, n = err.x[None], err.y[None], [len(err.x)]
    scale = np.array([err.nu / LAMBDA])
    centre = hip_engine.spot_radii(x, y, n, (1.0,))[0] * scale[0]
    freq, sag, tan = ort.geo_mtf(err, engine=hip_engine)
    m, _ = hip_engine.geo_mtf(x, y, n, 128, 2.0 / 128, scale=scale, centre=centre)
    assert np.array_equal(freq, ort.mtf_frequencies(128)) and np.array_equal(sag, m[0, 0]) and np.array_equal(tan, m[0, 1])
    assert sag[0] == 1.0 and tan[0] == 1.0 and sag[1:].max() <= 1.0 and tan[1:].max() <= 1.0
    image, lsf, outside = ort.spot_image(err, engine=hip_engine)
    want = hip_engine.spot_image(x, y, n, 64, 0.125, scale=scale, centre=centre)
    assert np.array_equal(image, want[0][0]) and np.array_equal(lsf, want[1][0]) and outside == want[2][0]
    assert image.shape == (64, 64) and image.sum() + outside == n[0]


@pytest.mark.parametrize("kw", (dict(nfreq=0), dict(nfreq=513), dict(dnu=0.0), dict(dnu=-1.0), dict(dnu=float("nan")),
                                dict(nimg=0), dict(nimg=24), dict(nimg=144), dict(dxi=0.0), dict(dxi=float("nan")), dict(cap=0)))
def test_bad_arguments(hip_engine, kw):
    z = np.zeros((1, kw.get("cap", 8)))
    with pytest.raises(_capi.OrtError) as e:
        if "nimg" in kw or "dxi" in kw:
            hip_engine.spot_image(z, z, [8], kw.get("nimg", 16), kw.get("dxi", 1.0))
        else:
            hip_engine.geo_mtf(z, z, [8], kw.get("nfreq", 16), kw.get("dnu", 0.5))
    assert e.value.code == -1                                         # ORT_EINVAL
    if kw == dict(cap=0):                                             # NULL pointers, no output, nb < 0, cap >= 2^31; both families
        lib, h = hip_engine.ctx.lib, hip_engine.ctx.h
        z, count, room = np.zeros((1, 8)), np.array([8], dtype=np.int64), np.zeros(16 * 16)       # (kept alive: the calls write)
        p, cnt, out = z.ctypes.data, count.ctypes.data, room.ctypes.data
        with pytest.raises(_capi.OrtError):
            hip_engine.spot_image(z[:, :0], z[:, :0], [0], 16, 1.0)
        for f64, f32, tail in ((lib.ort_geo_mtf_f64, lib.ort_geo_mtf_f32, [16, 0.5, None, out, 0]),
                               (lib.ort_spot_image_f64, lib.ort_spot_image_f32, [16, 1.0, out, None, None, 0])):
            good = [h, 1, 8, cnt, p, p, None, None] + tail
            assert f64(*good) == 0 and f32(*good) == 0
            for i in (3, 4, 5):
                assert f64(*(None if j == i else v for j, v in enumerate(good))) == -1
            assert f32(*(None if j in (10, 11) else v for j, v in enumerate(good))) == -1
            assert f64(h, -1, *good[2:]) == -1 and f32(h, 1, 2 ** 31, *good[3:]) == -1
