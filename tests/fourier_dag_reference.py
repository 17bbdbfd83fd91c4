"""NumPy interpreter of the tables of ``qmle_fourier_dag``, written from the description in ``include/qmle_sv.h`` -- a
loop over the levels and their nodes, one node at a time -- and independent of the package's own host path
(``FourierTree._evaluate_host``).  ``absolute=True`` walks the same DAG with ``|cos|``, ``|sin|`` and every power of i
replaced by 1: the result ``A(omega) = sum over paths of |weight|`` bounds the rounding error of a float64 walk, which
is at most ``8 P 2^-53 A(omega)`` for P levels (each level costs one complex multiply-add of a 2-ulp sine / cosine).

Also here: the dense complex128 yardstick ``<0| U^+ O U |0>`` of a recorded tape, built from ``Operation.matrix``.
"""
import numpy as np

ONE, ZERO = -1, -2
ANGLE, SHIFT = 0, 1
NODE = np.dtype([("cos_child", "<i4"), ("sin_child", "<i4"), ("power", "<i4"), ("pad", "<i4")])
LEVEL = np.dtype([("node_begin", "<i4"), ("node_end", "<i4"), ("kind", "<i4"), ("column", "<i4"), ("axis", "<i4"),
                  ("shift", "<i4")])


def make_nodes(rows):
    """``[(cos_child, sin_child, power), ...]`` -> node records."""
    out = np.zeros(len(rows), dtype=NODE)
    for j, (c, s, p) in enumerate(rows):
        out[j] = (c, s, p, 0)
    return out


def make_levels(rows):
    """``[(node_begin, node_end, "angle", column) | (node_begin, node_end, "shift", axis, shift), ...]``."""
    out = np.zeros(len(rows), dtype=LEVEL)
    for l, r in enumerate(rows):
        out[l] = (r[0], r[1], ANGLE, r[3], 0, 0) if r[2] == "angle" else (r[0], r[1], SHIFT, 0, r[3], r[4])
    return out


def _moved(f, dims, axis, w):
    """(T f)(omega) = f(omega - w e_axis) on the grid ``dims``, zero where omega - w e_axis is outside.  f: [B, F]."""
    g = f.reshape((f.shape[0],) + tuple(dims))
    out = np.zeros_like(g)
    n = dims[axis]
    for i in range(n):
        if 0 <= i - w < n:
            out[(slice(None),) * (1 + axis) + (i,)] = g[(slice(None),) * (1 + axis) + (i - w,)]
    return out.reshape(f.shape)


def interpret(nodes, levels, roots, root_phase, dims, angles, absolute=False):
    """-> ``[B, n_roots, F]`` (complex128; float64 with ``absolute``)."""
    dims = [int(d) for d in dims]
    F = int(np.prod(dims)) if dims else 1
    angles = np.asarray(angles, dtype=np.float64).reshape(len(angles), -1)
    B = angles.shape[0]
    dtype = np.float64 if absolute else np.complex128
    strides = [int(np.prod(dims[a + 1:])) for a in range(len(dims))]
    centre = sum((n - 1) // 2 * s for n, s in zip(dims, strides))
    unit = np.zeros((B, F), dtype=dtype)
    unit[:, centre] = 1.0
    zero = np.zeros((B, F), dtype=dtype)
    V = [None] * len(nodes)

    def value(code):
        return unit if code == ONE else zero if code == ZERO else V[code]

    def i_pow(k):
        return 1.0 if absolute else 1j ** (k % 4)

    for lv in levels:
        for j in range(int(lv["node_begin"]), int(lv["node_end"])):
            a, b, p = value(int(nodes[j]["cos_child"])), value(int(nodes[j]["sin_child"])), int(nodes[j]["power"])
            if lv["kind"] == ANGLE:
                c, s = np.cos(angles[:, lv["column"]])[:, None], np.sin(angles[:, lv["column"]])[:, None]
                if absolute:
                    c, s = np.abs(c), np.abs(s)
                V[j] = c * a + i_pow(1 + p) * s * b
            else:
                axis, w = int(lv["axis"]), int(lv["shift"])
                minus = 1.0 if absolute else -1.0
                V[j] = 0.5 * (_moved(a, dims, axis, w) + _moved(a, dims, axis, -w)) \
                    + i_pow(p) * 0.5 * (_moved(b, dims, axis, w) + minus * _moved(b, dims, axis, -w))
    out = np.zeros((B, len(roots), F), dtype=dtype)
    for r, (code, ph) in enumerate(zip(roots, root_phase)):
        out[:, r] = i_pow(int(ph)) * value(int(code))
    return out


# ---- dense yardstick ---------------------------------------------------------------------------------------------
def dense_state(tape, n_qubits):
    """``U |0..0>`` of a recorded (unbatched) tape in complex128, gate by gate from ``Operation.matrix``."""
    from qml_essentials_amd.operations import Barrier, embed_matrix

    psi = np.zeros(2**n_qubits, dtype=np.complex128)
    psi[0] = 1.0
    wires = list(range(n_qubits))
    for o in tape:
        if isinstance(o, Barrier):
            continue
        psi = embed_matrix(np.asarray(o.matrix, dtype=np.complex128), o.wires, wires) @ psi
    return psi


def dense_expectations(tape, observables, n_qubits):
    """``[<0| U^+ O U |0>]`` for every observable, complex (the imaginary part of a Hermitian O is rounding)."""
    from qml_essentials_amd.operations import embed_matrix

    psi = dense_state(tape, n_qubits)
    wires = list(range(n_qubits))
    return np.array([np.vdot(psi, embed_matrix(np.asarray(o.matrix, dtype=np.complex128), o.wires, wires) @ psi)
                     for o in observables])
