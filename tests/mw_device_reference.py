"""A plain float64 reference for Meyer-Wallach on whatever device the states live on (test infrastructure).

``purities_and_q`` restates ``oracle.analysis.qubit_purities_pure`` in torch: per wire a = sum |psi|^2 over bit = 0, d
the same over bit = 1, c = sum psi_0 conj(psi_1), purity = a^2 + d^2 + 2 |c|^2, Q = 2 (1 - mean purity).  Every product
and every sum is float64.  The state is walked in blocks of ``block`` amplitudes so that the temporaries stay small at
any size (2^22 amplitudes: two blocks as float64 pairs, 64 MiB each, and a handful of float64 arrays of a block or
half a block -- some 250 MiB).  It imports nothing of the library under test.
"""
import torch

DEFAULT_BLOCK = 1 << 22


def purities_and_q(states, block=DEFAULT_BLOCK, return_parts=False):
    """states: [B, 2^n] complex64 (any device) -> (purities by wire [B, n], Q [B]), float64 on the same device.

    ``block``: amplitudes per step, a power of two.  A position p with 2^(p+1) <= block has both halves of every pair
    inside a block; above that a block lies wholly in bit = 0 or bit = 1 and its partner block 2^p amplitudes further.
    ``return_parts``: also the two parts of a purity beyond 1/2 for a normalised state, [B, n] each: the population
    part (a - d)^2 / 2 and the cross part 2 |c|^2."""
    assert states.dim() == 2 and states.dtype == torch.complex64, (states.shape, states.dtype)
    B, D = states.shape
    n = D.bit_length() - 1
    assert D == 1 << n and n >= 1 and block >= 2 and block & (block - 1) == 0, (D, block)
    block = min(block, D)
    lg = block.bit_length() - 1
    flat = torch.view_as_real(states)  # [B, D, 2] float32
    # sums[b, p] = (a, d, re c, im c) of bit position p
    sums = torch.zeros((B, n, 4), dtype=torch.float64, device=states.device)
    for b in range(B):
        for k in range(D // block):
            blk = flat[b, k * block:(k + 1) * block].to(torch.float64)
            re, im = blk[:, 0], blk[:, 1]
            pr = re * re + im * im
            for p in range(lg):  # pairs inside the block
                lo = 1 << p
                r, i, q = re.view(-1, 2, lo), im.view(-1, 2, lo), pr.view(-1, 2, lo)
                sums[b, p, 0] += q[:, 0].sum()
                sums[b, p, 1] += q[:, 1].sum()
                sums[b, p, 2] += (r[:, 0] * r[:, 1] + i[:, 0] * i[:, 1]).sum()
                sums[b, p, 3] += (i[:, 0] * r[:, 1] - r[:, 0] * i[:, 1]).sum()
            tot = pr.sum()
            for p in range(lg, n):  # the block index carries the bit
                if (k >> (p - lg)) & 1:
                    sums[b, p, 1] += tot
                    continue
                sums[b, p, 0] += tot
                k1 = k + (1 << (p - lg))
                other = flat[b, k1 * block:(k1 + 1) * block].to(torch.float64)
                sums[b, p, 2] += (re * other[:, 0] + im * other[:, 1]).sum()
                sums[b, p, 3] += (im * other[:, 0] - re * other[:, 1]).sum()
    a, d = sums[..., 0], sums[..., 1]
    cross = 2.0 * (sums[..., 2] ** 2 + sums[..., 3] ** 2)
    by_wire = torch.flip(a * a + d * d + cross, dims=[1])  # wire w sits at bit position n - 1 - w
    q = 2.0 * (1.0 - by_wire.mean(dim=1))
    if return_parts:
        return by_wire, q, torch.flip(0.5 * (a - d) ** 2, dims=[1]), torch.flip(cross, dims=[1])
    return by_wire, q
