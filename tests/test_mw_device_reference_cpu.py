"""tests/mw_device_reference.py on CPU tensors against the oracle's Meyer-Wallach (oracle/analysis.py): the float64
reference that the GPU tests of the fused route use above 22 qubits, where no host reference is affordable."""
import numpy as np
import pytest
import torch

from oracle import analysis as OA
from tests.mw_device_reference import DEFAULT_BLOCK, purities_and_q

TOL = 1e-12


def random_states(n, batch, seed):
    """normalised complex64 states with unequal populations and a large cross term on every wire: a product state
    of random single-wire states (0.15 <= |amplitude of 1|^2 <= 0.4) plus a random perturbation"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(batch):
        psi = np.ones(1, dtype=np.complex128)
        for _ in range(n):
            p1 = rng.uniform(0.15, 0.4)
            psi = np.kron(psi, np.array([np.sqrt(1 - p1), np.sqrt(p1) * np.exp(1j * rng.uniform(0, 2 * np.pi))]))
        psi = psi + 0.3 * (rng.normal(size=psi.shape) + 1j * rng.normal(size=psi.shape)) / np.sqrt(2.0 * psi.size)
        out.append(psi / np.linalg.norm(psi))
    return np.stack(out).astype(np.complex64)


# (n, block): the default block holds every state here whole; the smaller ones split the state -- one block per
# amplitude pair, several positions above the block, and a block of the whole state minus one position
CASES = [(1, DEFAULT_BLOCK), (2, DEFAULT_BLOCK), (2, 2), (5, DEFAULT_BLOCK), (5, 4), (11, DEFAULT_BLOCK), (11, 1 << 10),
         (13, DEFAULT_BLOCK), (13, 1 << 6), (13, 1 << 12)]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n,block", CASES)
def test_reference_matches_the_oracle(n, block, batch):
    st = random_states(n, batch, 7 * n + batch)
    pur, q, pop, cross = purities_and_q(torch.from_numpy(st), block=block, return_parts=True)
    assert pur.dtype == torch.float64 and pur.shape == (batch, n) and q.shape == (batch,)
    st128 = st.astype(np.complex128)
    want_p = np.stack([OA.qubit_purities_pure(v, n) for v in st128])
    want_q = np.array([OA.meyer_wallach_pure(v, n) for v in st128])
    assert np.abs(pur.numpy() - want_p).max() < TOL
    assert np.abs(q.numpy() - want_q).max() < TOL
    # the parts: with a + d = 1 a purity is 1/2 + population part + cross part (complex64 states: norm to ~1e-7)
    assert np.abs(0.5 + pop.numpy() + cross.numpy() - want_p).max() < 1e-6
    if n >= 5:  # the states are a probe of both parts
        assert pop.min() > 1e-3 and cross.min() > 1e-3
    plain = purities_and_q(torch.from_numpy(st), block=block)
    assert len(plain) == 2 and torch.equal(plain[0], pur) and torch.equal(plain[1], q)


def test_the_split_is_taken():
    """a block smaller than the state walks more than one block: the answers of two block sizes differ in the last
    bits only (another order of the same float64 sums), and a block that is no power of two is refused"""
    st = torch.from_numpy(random_states(13, 1, 99))
    whole, split = purities_and_q(st), purities_and_q(st, block=1 << 6)
    assert float((whole[0] - split[0]).abs().max()) < TOL
    with pytest.raises(AssertionError):
        purities_and_q(st, block=96)
