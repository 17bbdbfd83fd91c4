"""Bit-level record of the Meyer-Wallach paths: ``python tools/mw_corpus.py [--lib PATH] [--out FILE]`` (needs a GPU).

One line per case -- n, batch, Hardware-Efficient layers, switch, then the SHA-256 of the float32 bytes of
``plan.run(angles, "mw")`` and of ``meyer_wallach(states, return_purities=True)`` on the states the same plan stores
-- and a last line with the digest over all lines.  The paths use no atomics, so two runs of one library give the
same file, and two libraries that launch the same kernels with the same arguments give the same file: ``cmp`` the
outputs of a build before and after a change to the host path.

n = 3, 11 (per-wire sweeps; whole-state plans), 12, 13 (one read; whole-state plans), 16, 17, 20, 21, 24 (tiled: the
fused route's column finish, one and two later reads, an odd run, overlapping runs); batch 1 and 3; one and two
layers; the default, ``QMLE_MW_NO_LEAN=1`` and ``QMLE_MW_FUSE_TILED=0``.
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from qml_essentials_amd import _native as N  # noqa: E402

SWITCHES = (("default", None), ("no_lean", ("QMLE_MW_NO_LEAN", "1")), ("standalone", ("QMLE_MW_FUSE_TILED", "0")))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def main(argv):
    out = sys.stdout
    import torch  # (before the library: it must resolve torch's HIP runtime, not a second one)

    if "--lib" in argv:
        import ctypes

        N.LIB_PATH = os.path.abspath(argv[argv.index("--lib") + 1])
        handle = ctypes.CDLL(N.LIB_PATH)
        N.SYMBOLS = [s for s in N.SYMBOLS if hasattr(handle, s[0])]  # (an older library lacks the newer entries)
    if "--out" in argv:
        out = open(argv[argv.index("--out") + 1], "w")
    from tests.test_abi_cpu import he_layer_ops

    total = hashlib.sha256()
    for n in (3, 11, 12, 13, 16, 17, 20, 21, 24):
        for layers in (1, 2):
            ops, slots = [], 0
            for _ in range(layers):
                o, sl = he_layer_ops(n)
                ops += [(g, w, [x + slots for x in k], m) for g, w, k, m in o]
                slots += sl
            plan = N.Plan(ops, n, slots)
            for batch in (1, 3):
                rng = np.random.default_rng(1000 * n + 10 * layers + batch)
                ang = torch.from_numpy(rng.uniform(0, 2 * np.pi, (batch, slots)).astype(np.float32)).cuda()
                states = plan.run(ang, "state")
                for name, switch in SWITCHES:
                    if switch:
                        os.environ[switch[0]] = switch[1]
                    try:
                        fused = plan.run(ang, "mw").cpu().numpy()
                        q, pur = N.meyer_wallach(states, return_purities=True)
                    finally:
                        if switch:
                            del os.environ[switch[0]]
                    alone = np.concatenate([q.cpu().numpy()[:, None], pur.cpu().numpy()], axis=1)
                    line = "n %d batch %d layers %d %s %s %s\n" % (n, batch, layers, name, sha(fused), sha(alone))
                    total.update(line.encode())
                    out.write(line)
                    out.flush()
    out.write("digest %s\n" % total.hexdigest())
    if out is not sys.stdout:
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
