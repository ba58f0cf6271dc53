"""Centre of mass, centroidal momentum / energy and the centroidal momentum matrix on the GPU:
multibody_com_batch_* / multibody_centroidal_batch_* / multibody_cmm_batch_* against
tests/centroidal_ref.py (the header's definitions on the 6x6 model's own joint transforms and link
inertias).  Every batch is B = 257 -- one full 256-lane block and a one-lane tail -- on rows of leading
dimension B + 37 (FR3 also B = 1 and 255).  Bounds: the header's (fp64 1e-9 scaled against the
reference; the identities with the project's own kernels 1e-12, the gravity identity 1e-9; host and
device lane bodies 1e-12; fp32 1e-4 norm-wise, the link_kin / contact_wrench contract).

Measured on MI355X (this file's own prints): fp64 against the reference 1.4e-15 FR3, 2.2e-14 16 links,
6.3e-15 general5, 1.9e-15 tree9, 1.2e-14 floating14 (the largest is energy or hg each time); A_G qd
2.0e-14 at most (floating14), T against crba_batch 3.4e-15, gravity 9.4e-14 (chain16), U exact, the
floating base's translation columns 9.9e-15; host against device lane body 2.2e-15; fp32 against the
fp64 kernel 1.2e-6 at most (general5 energy)."""
import numpy as np
import pytest

import centroidal_ref as cz
import ext_wrench_ref as xr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

B, LD = 257, 257 + 37
SENTINEL = -7.25
G = 9.81
MODELS = ["fr3", "chain16", "general5", "tree9", "floating14"]
_cache = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from rigidbody_amd import ffi

    if not hasattr(ffi.Multibody, "centroidal_batch"):
        pytest.fail("the binding has no centroidal entry points")
    return torch.device("cuda:0")


def _case(case):
    """Model, inputs and reference of one case, computed once and never modified."""
    if case not in _cache:
        mb, om, m6 = xr.setup(case)
        q, qd = xr.inputs(mb, B, 81)[:2]
        ref = (*cz.centroidal_batch(m6, q, qd), cz.cmm_batch(m6, q))
        _cache[case] = dict(mb=mb, m6=m6, x=(q, qd), ref=ref)
        for a in (q, qd, *ref):
            a.setflags(write=False)
    return _cache[case]


def _t(a, dev, dtype=torch.float64, fill=0.0, ld=LD):
    """[rows, b] view of a [rows, ld] device tensor whose padding columns hold `fill`."""
    a = np.array(a)  # a writable copy: the cached inputs are read-only
    b = a.shape[1]
    t = torch.full((a.shape[0], ld), fill, dtype=dtype, device=dev)
    t[:, :b] = torch.as_tensor(a, dtype=dtype, device=dev)
    return t[:, :b]


def _padded_out(rows, dev, dtype=torch.float64, b=B, ld=LD):
    full = torch.full((rows, ld), SENTINEL, dtype=dtype, device=dev)
    return full, full[:, :b]


def _scaled(got, ref):
    got = np.asarray(got, float)
    assert np.all(np.isfinite(got)), "non-finite output"
    return (np.abs(got - ref) / (1.0 + np.abs(ref))).max()


def _all(mb, q, qd):
    """(com of com_batch, com, hg, energy of centroidal_batch, ag of cmm_batch)."""
    return (mb.com_batch(q), *mb.centroidal_batch(q, qd), mb.cmm_batch(q))


def _check_parity(case, dev, b, ld):
    c = _case(case)
    mb, n = c["mb"], c["mb"].n
    q, qd = (_t(a[:, :b], dev, ld=ld) for a in c["x"])
    assert b == 1 or q.stride(0) == ld
    rows = (3, 3, 6, 2, 6 * n)
    outs = [_padded_out(r, dev, b=b, ld=ld) for r in rows]
    com0, com, hg, en, ag = (o[1] for o in outs)
    mb.com_batch(q, out=com0)
    mb.centroidal_batch(q, qd, com=com, hg=hg, energy=en)
    mb.cmm_batch(q, out=ag)
    refs = (c["ref"][0], *c["ref"])
    errs = [_scaled(t.cpu().numpy(), r[:, :b]) for t, r in zip((com0, com, hg, en, ag), refs)]
    print(f"{case} B={b} f64: com {max(errs[:2]):.3e} hg {errs[2]:.3e} energy {errs[3]:.3e} ag {errs[4]:.3e}")
    assert max(errs) <= 1e-9
    for full, _ in outs:  # columns past the batch are untouched
        assert bool((full[:, b:] == SENTINEL).all())
    assert torch.equal(com0, com)
    return q, qd, (com0, com, hg, en, ag)


@pytest.mark.parametrize("case", MODELS)
def test_parity_f64(case, dev):
    q, qd, (com0, com, hg, en, ag) = _check_parity(case, dev, B, LD)
    mb = _case(case)["mb"]
    # outputs the binding allocates share the inputs' leading dimension
    got = _all(mb, q, qd)
    assert all(g.stride(0) == LD for g in got)
    for g, w in zip(got, (com0, com, hg, en, ag)):
        assert torch.equal(g, w)


@pytest.mark.parametrize("b", [1, 255])
def test_parity_f64_small_batches(b, dev):
    _check_parity("fr3", dev, b, b + 37)


@pytest.mark.parametrize("case", MODELS)
def test_identities_with_the_projects_kernels(case, dev):
    """hg = A_G qd; T = 1/2 qd^T sym(H) qd with H of crba_batch; A_G[0:3]^T (0, 0, g) = rnea_batch(q, 0, 0);
    U = g M com_z; a floating base's translation columns of A_G are [M 1; 0]."""
    c = _case(case)
    mb, n, M = c["mb"], c["mb"].n, c["mb"].total_mass
    q, qd = (_t(a, dev) for a in c["x"])
    _, com, hg, en, ag = (t.cpu().numpy() for t in _all(mb, q, qd))
    A = ag.reshape(n, 6, B).transpose(1, 0, 2)  # [row, col, b]
    qdn = c["x"][1]
    e0 = _scaled(np.einsum("rkb,kb->rb", A, qdn), hg)
    H = mb.crba_batch(q).cpu().numpy().reshape(n, n, B).transpose(1, 0, 2)  # [row, col, b], upper triangle
    up, strict = np.triu(np.ones((n, n)))[:, :, None], np.triu(np.ones((n, n)), 1)[:, :, None]
    Hs = H * up + (H * strict).transpose(1, 0, 2)
    e1 = _scaled(0.5 * np.einsum("ib,ijb,jb->b", qdn, Hs, qdn), en[0])
    z = _t(np.zeros((n, B)), dev)
    grav = mb.rnea_batch(q, z, z).cpu().numpy()
    e2 = _scaled(G * A[2], grav)
    e3 = _scaled(en[1], G * M * com[2])
    print(f"{case} identities: A_G qd {e0:.3e} T {e1:.3e} gravity {e2:.3e} U {e3:.3e}")
    assert e0 <= 1e-12 and e1 <= 1e-12 and e2 <= 1e-9 and e3 <= 1e-15
    if case == "floating14":
        par, typ = mb.topology()
        assert list(typ[:3]) == [1, 1, 1]  # the virtual prismatic x, y, z
        want = np.zeros((6, 3, B))
        for k in range(3):
            want[k, k] = M
        e4 = _scaled(A[:, :3], want)
        print(f"{case} translation columns {e4:.3e}")
        assert e4 <= 1e-12


def test_host_and_device_lane_bodies_agree(dev):
    """The kernel against the single-configuration host form of the same lane body, FR3, 64 configurations."""
    c = _case("fr3")
    mb = c["mb"]
    nb = 64
    q, qd = (_t(a[:, :nb], dev, ld=nb) for a in c["x"])
    com0, com, hg, en, ag = (t.cpu().numpy() for t in _all(mb, q, qd))
    worst = 0.0
    for b in range(nb):
        qb, qdb = c["x"][0][:, b], c["x"][1][:, b]
        h_com, h_hg, h_en = mb.centroidal(qb, qdb)
        for got, want in ((com0[:, b], mb.com(qb)), (com[:, b], h_com), (hg[:, b], h_hg), (en[:, b], h_en),
                          (ag[:, b], mb.cmm_raw(qb))):
            worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print(f"fr3 host / device lane bodies {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("case", ["fr3", "general5", "tree9", "floating14"])
def test_f32_against_f64_kernel(case, dev):
    c = _case(case)
    mb = c["mb"]
    q, qd = (a.astype(np.float32).astype(np.float64) for a in c["x"])
    got = _all(mb, _t(q, dev, torch.float32), _t(qd, dev, torch.float32))
    ref = _all(mb, _t(q, dev), _t(qd, dev))
    for name, g, r in zip(("com", "com", "hg", "energy", "ag"), got, ref):
        g, r = g.cpu().numpy().astype(np.float64), r.cpu().numpy()
        assert np.all(np.isfinite(g))
        e = np.abs(g - r).max(axis=0) / (1 + np.abs(r).max(axis=0))
        print(f"{case} {name} f32 norm-wise {e.max():.3e} at configuration {e.argmax()}")
        assert e.max() <= 1e-4


@pytest.mark.parametrize("case", ["fr3", "floating14"])
def test_host_pointer_forms_equal_device_forms(case, dev):
    c = _case(case)
    mb = c["mb"]
    q, qd = c["x"]
    for npd, dtype in ((np.float64, torch.float64), (np.float32, torch.float32)):
        want = _all(mb, _t(q, dev, dtype), _t(qd, dev, dtype))
        got = (mb.com_batch_host(q, dtype=npd), *mb.centroidal_batch_host(q, qd, dtype=npd),
               mb.cmm_batch_host(q, dtype=npd))
        for g, w in zip(got, want):
            assert g.dtype == npd and np.array_equal(g, w.cpu().numpy())


@pytest.mark.parametrize("case", ["fr3", "floating14"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_input_domain(case, dtype, dev):
    """NaN in q, Inf in qd and an angle of 2^42 rad in three configurations: NaN in every output element
    that reads the bad input, every other configuration bit-identical to the clean run."""
    c = _case(case)
    mb = c["mb"]
    td = torch.float64 if dtype == "f64" else torch.float32
    q, qd = (_t(a, dev, td) for a in c["x"])
    clean = _all(mb, q, qd)
    par, typ = mb.topology()
    rev = int(np.flatnonzero(typ == 0)[1])  # a revolute joint (an angle); row 0 is prismatic on a floating base
    qb, qdb = q.clone(), qd.clone()
    qb[0, 5] = float("nan")
    qdb[mb.n - 1, 130] = float("inf")
    qb[rev, 256] = 2.0 ** 42
    outs = _all(mb, qb, qdb)
    keep = np.ones(B, bool)
    keep[[5, 130, 256]] = False
    for k, (got, ref) in enumerate(zip(outs, clean)):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert np.isnan(got[:, 5]).all() and np.isnan(got[:, 256]).all(), k
        if k in (1, 2, 3):  # centroidal_batch reads qd
            assert np.isnan(got[:, 130]).all(), k
        else:
            assert np.array_equal(got[:, 130], ref[:, 130]), k
        assert np.array_equal(got[:, keep], ref[:, keep]), k
        assert np.all(np.isfinite(ref)), k


def test_graph_capture(dev):
    """One centroidal_batch (a single kernel) captured after upload() and a warm-up call, replayed once."""
    c = _case("fr3")
    mb = c["mb"]
    q, qd = (_t(a, dev) for a in c["x"])
    mb.upload()
    eager = mb.centroidal_batch(q, qd)  # also compiles the kernel before the capture
    torch.cuda.synchronize(dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = mb.centroidal_batch(q, qd)
    for o in out:
        o.zero_()
    g.replay()
    torch.cuda.synchronize(dev)
    for o, e in zip(out, eager):
        assert torch.equal(o, e)


def test_without_hiprtc_fails_loudly(dev):
    from rigidbody_amd import ffi

    mb = _case("fr3")["mb"]
    z = torch.zeros((mb.n, 8), dtype=torch.float64, device=dev)
    try:
        ffi.set_tuning("jit", 0)
        for call in (lambda: mb.com_batch(z), lambda: mb.centroidal_batch(z, z), lambda: mb.cmm_batch(z)):
            with pytest.raises(ffi.RigidBodyError, match="hipRTC"):
                call()
    finally:
        ffi.set_tuning("jit", 1)
