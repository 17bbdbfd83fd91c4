"""Every dispatch branch of the stand-alone measurement and analysis kernels (csrc/qmle_analysis.hip) and of
the Gram kernels (csrc/qmle_gram.hip) against a plain float64 / complex128 NumPy reference.

Each entry point picks its launch shape or algorithm on the host from the register size, the batch or the
argument count.  Every test states which branch its sizes take -- from the library's own workspace query
where one exists, from the host code's rule otherwise -- and the sweeps assert that both sides of every
threshold are taken, so that a retune cannot silently stop covering a branch.  Inputs are complex64 states
(what the kernels read); the references take those same values in complex128."""
import ctypes as C

import numpy as np
import pytest

from oracle import analysis as OA

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -10
QMLE_MAX_QUBITS = 32


def _N():
    from qml_essentials_amd import _native as N

    return N


def _states(rng, B, n):
    """Seeded random normalised states [B, 2^n] (complex64 values held in complex128), made non-uniform --
    amplitude decay plus wire-dependent scaling -- so that a wrong index bit or sign changes the answer."""
    D = 1 << n
    idx = np.arange(D)
    shape = np.exp(-idx / D)
    for k in range(0, n, 3):
        shape *= np.where((idx >> k) & 1, 1.0 + 0.15 * k, 1.0)
    st = np.empty((B, D), dtype=np.complex64)
    st.real = rng.standard_normal((B, D), dtype=np.float32)
    st.imag = rng.standard_normal((B, D), dtype=np.float32)
    st = st.astype(np.complex128) * shape[None, :]
    st /= np.linalg.norm(st, axis=1, keepdims=True)
    return st.astype(np.complex64).astype(np.complex128)


def _dev(st):
    return torch.from_numpy(np.ascontiguousarray(st.astype(np.complex64))).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ---- histogram ------------------------------------------------------------------------------------------
HIST_BINS = [1, 3, 7, 75, 100, 300, 4096, 4097, 10000]
HIST_RANGES = [(0.0, 1.0), (-1.0, 1.0), (0.1, 0.7)]


def _hist_path(count, n_bins):
    """qmle_histogram's launch (csrc/qmle_analysis.hip, qmle_histogram)."""
    if n_bins <= 4096 and 0 < count <= 1 << 16:
        return "lds_solo"       # k_histogram_lds<true>: one workgroup, bins stored
    return "lds_multi" if n_bins <= 4096 else "global"  # k_histogram_lds<false> / k_histogram


def _edge_values(lo, hi, n_bins, ulps=3):
    """Every float32 within +-ulps of every edge of linspace(f32(lo), f32(hi), n_bins + 1), exactly lo and hi,
    values just outside the range, NaN and +-inf."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    e = np.linspace(float(lo32), float(hi32), n_bins + 1).astype(np.float32)
    v = [e]
    down, up = e.copy(), e.copy()
    for _ in range(ulps):
        down = np.nextafter(down, np.float32(-np.inf))
        up = np.nextafter(up, np.float32(np.inf))
        v += [down, up]
    v.append(np.array([lo32, hi32, np.nextafter(lo32, np.float32(-np.inf)), np.nextafter(hi32, np.float32(np.inf)),
                       lo32 - 0.5, hi32 + 0.5, np.nan, np.inf, -np.inf], dtype=np.float32))
    return np.concatenate(v)


def _hist_want(values, lo, hi, n_bins):
    """np.histogram with the float64 edges np.linspace computes from the float32 range the kernel receives."""
    edges = np.linspace(float(np.float32(lo)), float(np.float32(hi)), n_bins + 1)
    return np.histogram(values, bins=edges)[0]


def _hist_sizes(base, n_bins):
    """The value set as it is, and tiled past 65 536 values; paths each size takes."""
    tiled = np.tile(base, (1 << 16) // base.size + 2)
    assert base.size <= 1 << 16 and tiled.size > 1 << 16
    return [base, tiled]


@pytest.mark.parametrize("lo,hi", HIST_RANGES)
@pytest.mark.parametrize("n_bins", HIST_BINS)
def test_histogram_edges_equal_numpy_float64_edges_on_every_path(n_bins, lo, hi):
    N = _N()
    base = _edge_values(lo, hi, n_bins)
    rng = np.random.default_rng(n_bins)
    base = base[rng.permutation(base.size)]  # (edge values spread over the threads / workgroups)
    if base.size > 1 << 16:  # (10 000 bins: 70 000 edge values) -- the single-workgroup path gets a share
        sets = [base[: 1 << 16], base]
    else:
        sets = _hist_sizes(base, n_bins)
    for v in sets:
        got = N.histogram(torch.from_numpy(v).cuda(), n_bins, lo, hi).cpu().numpy()
        want = _hist_want(v, lo, hi, n_bins)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (_hist_path(v.size, n_bins), v.size, bad[:8], got[bad[:8]], want[bad[:8]])


def test_histogram_sweep_takes_every_path():
    taken = set()
    for n_bins in HIST_BINS:
        for lo, hi in HIST_RANGES:
            base = _edge_values(lo, hi, n_bins)
            sets = [base[: 1 << 16], base] if base.size > 1 << 16 else _hist_sizes(base, n_bins)
            taken |= {_hist_path(v.size, n_bins) for v in sets}
    assert taken == {"lds_solo", "lds_multi", "global"}


def test_expressibility_histogram_equals_the_oracle_on_the_same_fidelities(monkeypatch):
    """Expressibility.state_fidelities bins on the GPU; the counts equal OA.fidelity_histogram of the very
    fidelities it binned, pulled back to the host."""
    from qml_essentials_amd.expressibility import Expressibility
    from qml_essentials_amd.model import Model

    seen = []
    orig = Expressibility._sample_state_fidelities.__func__

    def spy(cls, *a, **kw):
        fid = orig(cls, *a, **kw)
        seen.append(fid.detach().cpu().numpy().copy())
        return fid

    monkeypatch.setattr(Expressibility, "_sample_state_fidelities", classmethod(spy))
    model = Model(n_qubits=4, n_layers=2, circuit_type="Hardware_Efficient")
    for n_samples, n_bins in ((1000, 75), (3000, 100), (500, 7)):
        y, z = Expressibility.state_fidelities(n_samples=n_samples, n_bins=n_bins, model=model,
                                               random_key=np.random.default_rng(n_bins).integers(1 << 31))
        fid = seen.pop()
        y_want, z_want = OA.fidelity_histogram(fid.reshape(-1), n_bins, n_samples)
        np.testing.assert_array_equal(y, y_want)
        np.testing.assert_array_equal(np.asarray(z).reshape(-1), z_want)


# ---- <Z> on every wire ------------------------------------------------------------------------------------
EXPVAL_N = list(range(1, 25))


def _expval_blocks(n, B):
    """Blocks per state of k_expval_partial, read back from the workspace query (B * blocks * 33 floats)."""
    wsb = int(_N().lib().qmle_expval_workspace_bytes(n, B))
    return (wsb - 256) // (B * (QMLE_MAX_QUBITS + 1) * 4)


def _expval_path(n):
    nb, segs = _expval_blocks(n, 1), -(-(1 << (n - 1)) // 1024)
    assert nb == min(segs, 2048)
    return "one_segment" if segs == 1 else "segment_per_block" if segs <= 2048 else "capped_grid"


def _z_want(st, n):
    """<Z_w> for every wire w in float64: marginal of the wire's bit (wire 0 = most significant)."""
    p = np.abs(st) ** 2
    B = p.shape[0]
    return np.stack([(lambda m: m[:, 0] - m[:, 1])(p.reshape(B, 1 << w, 2, -1).sum(axis=(1, 3)))
                     for w in range(n)], axis=1)


@pytest.mark.parametrize("n", EXPVAL_N)
def test_expval_z_every_wire(n):
    N = _N()
    path = _expval_path(n)
    rng = np.random.default_rng(300 + n)
    B = 3 if n < 22 else 1
    st = _states(rng, B, n)
    wires = list(range(n))[::-1] + [0]  # every wire, out of order, one repeated
    got = N.expval_z(_dev(st), wires).cpu().numpy()
    want = _z_want(st, n)[:, wires]
    err = np.abs(got - want).max()
    assert err <= 1e-6, (path, err)


def test_expval_sweep_takes_every_path():
    assert {_expval_path(n) for n in EXPVAL_N} == {"one_segment", "segment_per_block", "capped_grid"}
    assert _expval_path(11) == "one_segment" and _expval_path(12) == "segment_per_block"
    assert _expval_path(22) == "segment_per_block" and _expval_path(23) == "capped_grid"


# ---- probabilities ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(1, 21)))
def test_probs_within_two_ulp(n):
    N = _N()
    rng = np.random.default_rng(400 + n)
    st = _states(rng, 3 if n <= 18 else 1, n)
    got = N.probs(_dev(st)).cpu().numpy().astype(np.float64)
    want = np.abs(st) ** 2
    assert np.all(np.abs(got - want) <= 2 * np.spacing(want.astype(np.float32)).astype(np.float64))


# ---- density matrices ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(1, 13)))
def test_density_every_element(n):
    N = _N()
    rng = np.random.default_rng(500 + n)
    st = _states(rng, 3, n)
    got = N.density(_dev(st)).cpu().numpy()
    for b in range(3):
        want = np.outer(st[b], st[b].conj())
        bound = 2.0 ** -22 * np.outer(np.abs(st[b]), np.abs(st[b]))
        assert np.all(np.abs(got[b] - want) <= bound), b


@pytest.mark.parametrize("n", [13, 14, 15])
def test_density_large_rows_against_a_complex128_outer_product_on_the_device(n):
    """D^2 threads are more than the grid cap (2^20 workgroups of 256) from n = 15: every row is checked, in
    blocks of rows, against the complex128 outer product formed on the device."""
    N = _N()
    rng = np.random.default_rng(600 + n)
    st = _dev(_states(rng, 1, n))
    got = N.density(st)[0]
    psi = st[0].to(torch.complex128)
    rows = 1024
    for r0 in range(0, 1 << n, rows):
        want = psi[r0:r0 + rows, None] * psi.conj()[None, :]
        bound = 2.0 ** -22 * (psi[r0:r0 + rows, None].abs() * psi.abs()[None, :])
        over = ((got[r0:r0 + rows].to(torch.complex128) - want).abs() > bound).sum().item()
        assert over == 0, (r0, over)
    del got
    torch.cuda.empty_cache()


def test_density_refuses_sixteen_qubits():
    """n = 16 returns QMLE_ERR_UNSUPPORTED before any launch (the wrapper would first allocate 32 GiB)."""
    N = _N()
    st = _dev(_states(np.random.default_rng(16), 1, 16))
    out = torch.zeros(16, dtype=torch.complex64, device="cuda")
    assert N.lib().qmle_density(_ptr(st), 16, 1, _ptr(out), N._stream_ptr()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not out.abs().any().item()


# ---- marginal probabilities -------------------------------------------------------------------------------------
MARGINAL_CASES = [(24, 1), (24, 12), (24, 13), (24, 24), (16, 13), (16, 14), (16, 15), (16, 16)]


def _marginal_path(n_keep):
    return "lds" if n_keep <= 12 else "global"  # k_marginal_lds / k_marginal (qmle_marginal_probs)


@pytest.mark.parametrize("n,n_keep", MARGINAL_CASES)
def test_marginal_probs_lds_and_global_atomics(n, n_keep):
    N = _N()
    rng = np.random.default_rng(700 + 32 * n + n_keep)
    st = _states(rng, 1 if n > 16 else 2, n)
    keep = [int(w) for w in rng.permutation(n)[:n_keep]]
    if n_keep > 1 and keep == sorted(keep):
        keep = keep[::-1]  # kept wires are passed in non-ascending order
    got = N.marginal_probs(_dev(st), keep).cpu().numpy()
    want = OA.marginalize_probs(np.abs(st) ** 2, n, keep)
    # float32 atomics add a bin's terms: 1e-6, or 4e-6 of the bin where that is larger (one kept wire of 24:
    # 2^23 terms per bin near 1/2, measured 1.02e-6)
    tol = np.maximum(1e-6, 4e-6 * want)
    err = np.abs(got - want)
    assert np.all(err <= tol), (_marginal_path(n_keep), keep, err.max())


def test_marginal_sweep_takes_both_paths():
    assert {_marginal_path(k) for _, k in MARGINAL_CASES} == {"lds", "global"}


# ---- pair fidelities ---------------------------------------------------------------------------------------------
PAIR_N = [1, 7, 8, 9, 16, 17, 20]
PAIR_COUNTS = [1, 63, 64, 300]
POOL = 11  # distinct states per call; the counts above are not multiples of it, so pair (i, i + S) mixes them


def _pair_path(n, pairs):
    """qmle_pair_fidelity: one workgroup per pair (n <= 16 and >= 64 pairs; 64 threads below 2^9 amplitudes),
    the two-launch form otherwise."""
    if n <= 16 and pairs >= 64:
        return "small_256" if n >= 9 else "small_64"
    return "two_launch"


@pytest.mark.parametrize("n", PAIR_N)
def test_pair_fidelity_both_paths(n):
    """States i and i + S of 2S rows, the rows drawn from a pool of 11 distinct states (the 600 rows of 2^20
    amplitudes would otherwise have to be generated on the host)."""
    N = _N()
    rng = np.random.default_rng(800 + n)
    pool = _states(rng, POOL, n)
    dpool = _dev(pool)
    for S in PAIR_COUNTS:
        idx = np.arange(2 * S) % POOL
        got = N.pair_fidelity(dpool[torch.from_numpy(idx).cuda()].contiguous()).cpu().numpy()
        ia, ib = idx[:S], idx[S:]
        want = OA.fidelities_pure(np.concatenate([pool[ia[:POOL]], pool[ib[:POOL]]]), min(S, POOL))
        want = want[np.arange(S) % POOL]
        err = np.abs(got - want).max()
        assert err <= 1e-6, (_pair_path(n, S), S, err)


def test_pair_fidelity_sweep_takes_every_path():
    paths = {(n, S): _pair_path(n, S) for n in PAIR_N for S in PAIR_COUNTS}
    assert set(paths.values()) == {"small_64", "small_256", "two_launch"}
    assert paths[(16, 63)] == "two_launch" and paths[(16, 64)] == "small_256"


# ---- overlaps ----------------------------------------------------------------------------------------------------
OVERLAP_N = list(range(1, 23))


def _overlap_blocks(n, count=1):
    wsb = int(_N().lib().qmle_overlap_workspace_bytes(n, count))
    return (wsb - 256) // (count * 8)


def _many(n):
    """The long batch: 1000 rows, fewer where two arrays of them would pass 4 GiB."""
    return min(1000, (1 << 28) >> n)


@pytest.mark.parametrize("n", OVERLAP_N)
def test_overlap_against_vdot(n):
    N = _N()
    rng = np.random.default_rng(900 + n)
    pool = _states(rng, 2 * POOL, n)
    dpool = _dev(pool)
    nb = _overlap_blocks(n)
    assert nb == min(1024, max(1, -(-(1 << (n - 1)) // 1024)))
    for count in (1, 3, _many(n)):
        ia, ib = np.arange(count) % POOL, POOL + (np.arange(count) * 3 + 1) % POOL
        a = dpool[torch.from_numpy(ia).cuda()].contiguous()
        b = dpool[torch.from_numpy(ib).cuda()].contiguous()
        got = N.overlap(a, b).cpu().numpy()
        k = min(count, POOL)
        want = np.array([np.vdot(pool[ia[i]], pool[ib[i]]) for i in range(k)])[np.arange(count) % k]
        err = np.abs(got - want).max()
        assert err <= 1e-6, (count, nb, err)


def test_overlap_sweep_reaches_the_block_cap():
    """One block at n <= 11, a block per 1024 float4 chunks up to n = 21, capped at 1024 with a grid-stride loop
    over 2048 chunk groups at n = 22."""
    assert _overlap_blocks(1) == 1 and _overlap_blocks(11) == 1 and _overlap_blocks(12) == 2
    assert _overlap_blocks(21) == 1024 and _overlap_blocks(max(OVERLAP_N)) == 1024


def test_overlap_raw_abi_past_one_launch_of_rows():
    """count = 65 537 through the C ABI: the kernel's own loop over launches of 65 535 rows (the Python
    wrapper cuts batches before they reach it)."""
    N = _N()
    n, count = 2, 65537
    rng = np.random.default_rng(65537)
    a_h, b_h = _states(rng, count, n), _states(rng, count, n)
    a, b = _dev(a_h), _dev(b_h)
    out = torch.zeros(count, dtype=torch.complex64, device="cuda")
    wsb = int(N.lib().qmle_overlap_workspace_bytes(n, count))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    assert N.lib().qmle_overlap(_ptr(a), _ptr(b), n, count, _ptr(out), _ptr(ws), wsb, N._stream_ptr()) == 0
    got = out.cpu().numpy()
    want = np.einsum("ij,ij->i", a_h.conj(), b_h)
    err = np.abs(got - want)
    assert err.max() <= 1e-6, (int(err.argmax()), err.max())


# ---- Z parities ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 12, 20])
@pytest.mark.parametrize("groups", [1, 8, 9, 17])
def test_expval_parity_groups_of_eight(n, groups):
    """Observables go 8 to a launch: 1, 8, 9 and 17 per call are one, one full, one full + one, and two
    full + one launch."""
    N = _N()
    rng = np.random.default_rng(1000 + 32 * n + groups)
    B = 3 if n <= 12 else 2
    st = _states(rng, B, n)
    wire_groups = []
    for k in range(groups):  # the full register (any order), a single wire, a random subset, in turn
        if k % 3 == 0:
            wire_groups.append([int(w) for w in rng.permutation(n)])
        elif k % 3 == 1:
            wire_groups.append([int(rng.integers(n))])
        else:
            wire_groups.append([int(w) for w in rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False)])
    got = N.expval_parity(_dev(st), wire_groups).cpu().numpy()
    p = np.abs(st) ** 2
    idx = np.arange(1 << n, dtype=np.uint64)
    want = np.empty((B, groups))
    for k, g in enumerate(wire_groups):
        bits = np.uint64(sum(1 << (n - 1 - w) for w in set(g)))
        sign = 1.0 - 2.0 * (np.bitwise_count(idx & bits) & 1)
        want[:, k] = p @ sign
    assert -(-groups // 8) == (1 if groups <= 8 else 2 if groups <= 16 else 3)
    err = np.abs(got - want).max()
    assert err <= 1e-6, (wire_groups, err)


# ---- measurements of vectorised density matrices -------------------------------------------------------------------
@pytest.mark.parametrize("n", list(range(1, 12)))
def test_density_probs_and_expval_of_mixed_states(n):
    """n = 11: one vec(rho) is 32 MiB, a batch of 2."""
    N = _N()
    rng = np.random.default_rng(1100 + n)
    B, K = (3 if n < 11 else 2), 4
    rho = np.zeros((B, 1 << n, 1 << n), dtype=np.complex128)
    for b in range(B):
        w = rng.random(K)
        w /= w.sum()
        psi = _states(rng, K, n)
        rho[b] = np.einsum("k,ki,kj->ij", w, psi, psi.conj())
    rho = rho.astype(np.complex64)
    dev = torch.from_numpy(rho.reshape(B, -1)).cuda()
    diag = np.real(np.einsum("bii->bi", rho)).astype(np.float64)
    got_p = N.density_probs(dev, n).cpu().numpy()
    np.testing.assert_array_equal(got_p, diag.astype(np.float32))  # a copy of the real diagonal
    wires = list(range(n))[::-1]
    got_z = N.density_expval_z(dev, n, wires).cpu().numpy()
    idx = np.arange(1 << n)
    want = np.stack([diag @ (1.0 - 2.0 * ((idx >> (n - 1 - w)) & 1)) for w in wires], axis=1)
    err = np.abs(got_z - want).max()
    assert err <= 1e-6, err


# ---- Gram matrices --------------------------------------------------------------------------------------------------
def _gram_want(a, b):
    a64, b64 = a.astype(np.complex128), b.astype(np.complex128)
    return np.conj(a64) @ np.swapaxes(b64, 1, 2), np.abs(a64) @ np.swapaxes(np.abs(b64), 1, 2)


def _gram_assert(got, a, b, f64):
    want, bound = _gram_want(a, b)
    if f64:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    else:
        assert np.all(np.abs(got - want) <= 1e-6 * bound + 1e-30)


def _rand(rng, shape, dtype):
    s = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    s /= np.linalg.norm(s, axis=-1, keepdims=True)
    return s.astype(dtype)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
@pytest.mark.parametrize("n", [5, 10])
def test_gram_general_form_ragged_tiles(n, dtype):
    """Rows 63 / 64 / 65 / 127 / 128 / 129 on either side (64-row tiles in complex64, 32-row tiles in
    complex128), in both orders; n = 5 stores straight from the tile kernel, n = 10 cuts rows into chunks and
    adds them in k_gram_reduce.  Equal row counts with a != b take the general form, not the Hermitian one."""
    N = _N()
    rng = np.random.default_rng(1200 + n)
    f64 = dtype == np.complex128
    wsq = N.lib().qmle_gram_workspace_bytes_f64 if f64 else N.lib().qmle_gram_workspace_bytes
    chunked = int(wsq(n, 2, 65, 129)) > 0
    assert chunked == (n == 10)
    rows = [63, 64, 65, 127, 128, 129]
    for ra, rb in [(63, 129), (129, 63), (64, 127), (127, 64), (65, 128), (128, 65), (65, 65), (128, 128)]:
        assert ra in rows and rb in rows
        a, b = _rand(rng, (2, ra, 1 << n), dtype), _rand(rng, (2, rb, 1 << n), dtype)
        got = N.gram(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        _gram_assert(got, a, b, f64)


def _gram_raw(fn, wsq, a, b, n, G, ra, rb, sa, sb, out):
    wsb = int(wsq(n, G, ra, rb))
    ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device="cuda")
    st = fn(_ptr(a), _ptr(b), n, G, ra, rb, sa, sb, _ptr(out), _ptr(ws), wsb, _stream_ptr())
    torch.cuda.synchronize()
    return st


def _stream_ptr():
    return _N()._stream_ptr()


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128])
def test_gram_group_strides_larger_than_the_rows(dtype):
    """Group strides of rows * d + padding through the C ABI, the padding NaN: any read outside the rows of a
    group would turn its entries into NaN.  General form and the Hermitian one (a is b, same stride)."""
    N = _N()
    f64 = dtype == np.complex128
    fn, wsq = ((N.lib().qmle_gram_f64, N.lib().qmle_gram_workspace_bytes_f64) if f64
               else (N.lib().qmle_gram, N.lib().qmle_gram_workspace_bytes))
    tdt = torch.complex128 if f64 else torch.complex64
    rng = np.random.default_rng(1300)
    for n, G, ra, rb, pad_a, pad_b in ((4, 3, 65, 31, 6, 100), (10, 2, 33, 70, 1024, 2), (13, 2, 9, 9, 8, 8)):
        d = 1 << n
        sa, sb = ra * d + pad_a, rb * d + pad_b
        a_h, b_h = _rand(rng, (G, ra, d), dtype), _rand(rng, (G, rb, d), dtype)
        a = torch.full((G * sa,), complex("nan"), dtype=tdt, device="cuda")
        b = torch.full((G * sb,), complex("nan"), dtype=tdt, device="cuda")
        for g in range(G):
            a[g * sa:g * sa + ra * d] = torch.from_numpy(a_h[g].reshape(-1)).cuda()
            b[g * sb:g * sb + rb * d] = torch.from_numpy(b_h[g].reshape(-1)).cuda()
        out = torch.empty((G, ra, rb), dtype=torch.complex128, device="cuda")
        assert _gram_raw(fn, wsq, a, b, n, G, ra, rb, sa, sb, out) == 0
        _gram_assert(out.cpu().numpy(), a_h, b_h, f64)
        herm = torch.empty((G, ra, ra), dtype=torch.complex128, device="cuda")
        assert _gram_raw(fn, wsq, a, a, n, G, ra, ra, sa, sa, herm) == 0
        got = herm.cpu().numpy()
        _gram_assert(got, a_h, a_h, f64)
        np.testing.assert_array_equal(got, np.conj(np.swapaxes(got, 1, 2)))


def test_gram_refuses_bad_arguments_on_the_host():
    """QMLE_ERR_INVALID_ARG, decided before any launch.  Every buffer is large enough for the call it is
    passed to, so a call that were accepted would still stay in bounds."""
    N = _N()
    fn, wsq = N.lib().qmle_gram, N.lib().qmle_gram_workspace_bytes
    n, d, G, R = 3, 8, 2, 4
    a = torch.zeros(G * R * d + 8, dtype=torch.complex64, device="cuda")
    out = torch.empty(4097 * 4097, dtype=torch.complex128, device="cuda")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def call(pa, ra, rb, sa, sb, groups=G):
        assert int(wsq(n, groups, ra, rb)) <= ws.numel()
        return fn(pa, pa, n, groups, ra, rb, sa, sb, _ptr(out), _ptr(ws), ws.numel(), _stream_ptr())

    assert call(_ptr(a), R, R, R * d, R * d) == 0  # the baseline call is accepted
    misaligned = C.c_void_p(a.data_ptr() + 8)  # one complex64 amplitude in: 8-byte aligned only
    assert a.data_ptr() % 16 == 0 and misaligned.value % 16 == 8
    assert call(misaligned, R, R, R * d, R * d) == ERR_INVALID_ARG
    assert call(_ptr(a), R, R, R * d + 1, R * d + 1) == ERR_INVALID_ARG       # odd complex64 stride
    big = torch.zeros(4097 * d, dtype=torch.complex64, device="cuda")
    assert fn(_ptr(big), _ptr(big), n, 1, 4097, 4097, 4097 * d, 4097 * d, _ptr(out), _ptr(ws), ws.numel(),
              _stream_ptr()) == ERR_INVALID_ARG                                 # 4097 rows
    assert call(_ptr(a), R, R, R * d - 2, R * d - 2) == ERR_INVALID_ARG       # stride < rows * d
    torch.cuda.synchronize()
