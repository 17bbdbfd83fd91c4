"""NumPy interpreter of the tables of ``qmle_compose_circuits`` (``include/qmle_sv.h``): a loop over circuits,
candidates and ops written from the definitions there, independent of ``qoc._op_matrices``.  ``longdouble=True`` runs
the same loop in extended precision (``clongdouble``), the yardstick for the float64 run's own rounding."""
import numpy as np

CONST, PULSE, ROT_X, ROT_Y, ROT_Z, CPHASE = range(6)
_SIGMA = {ROT_X: [[0, 1], [1, 0]], ROT_Y: [[0, -1j], [1j, 0]], ROT_Z: [[1, 0], [0, -1]]}


def _embedded(m, placement, ctype):
    """The d x d matrix of ``m`` under ``placement`` (wire 0 the most significant)."""
    eye = np.eye(2, dtype=ctype)
    if placement in (0, 3):
        return m
    if placement == 1:
        return np.kron(m, eye)
    if placement == 2:
        return np.kron(eye, m)
    if placement == 4:
        perm = [0, 2, 1, 3]  # |ab> <-> |ba>
        return m[np.ix_(perm, perm)]
    raise ValueError(f"placement {placement}")


def interpret(circuits, ops, terms, rows, n_candidates, mats, coefs, targets, jac, column_mask, longdouble=False):
    """-> per circuit ``dict(U [C, d, d], dU [C, P, d, d], ov [C] or None, dov [C, P] or None)``."""
    ctype = np.clongdouble if longdouble else np.complex128
    rtype = np.longdouble if longdouble else np.float64
    mats = None if mats is None else np.asarray(mats).reshape(-1).astype(ctype)
    coefs = None if coefs is None else np.asarray(coefs).reshape(-1).astype(rtype)
    targets = None if targets is None else np.asarray(targets).reshape(-1).astype(ctype)
    jac = None if jac is None else np.asarray(jac).reshape(-1, 6, 2, 2).astype(ctype)
    half_i = ctype(-0.5j)
    out = []
    for K in circuits:
        d, P = 2 ** int(K["n_wires"]), int(K["n_params"])
        U_all = np.zeros((n_candidates, d, d), dtype=ctype)
        dU_all = np.zeros((n_candidates, P, d, d), dtype=ctype)
        for c in range(n_candidates):
            U = np.eye(d, dtype=ctype)
            dU = np.zeros((P, d, d), dtype=ctype)
            for o in ops[int(K["op_begin"]):int(K["op_end"])]:
                kind, k = int(o["kind"]), 2 if int(o["placement"]) <= 2 else 4
                if kind == PULSE:
                    row = jac[int(rows[int(o["mat_off"]) + c])]
                    m = row[0]
                else:
                    at = int(o["mat_off"]) + c * int(o["mat_stride"])
                    m = mats[at:at + k * k].reshape(k, k)
                dm = np.zeros((P, k, k), dtype=ctype)
                for t in terms[int(o["term_begin"]):int(o["term_end"])]:
                    w = coefs[int(t["coef_off"]) + c]
                    if kind == PULSE:
                        g = row[1 + int(t["slot"])]
                    elif kind in _SIGMA:
                        g = half_i * (np.asarray(_SIGMA[kind], dtype=ctype) @ m)
                    elif kind == CPHASE:
                        g = np.zeros((4, 4), dtype=ctype)
                        g[3] = ctype(1j) * m[3]
                    else:
                        raise ValueError("a CONST op has no derivative")
                    dm[int(t["param"])] += w * g
                M = _embedded(m, int(o["placement"]), ctype)
                for p in range(P):
                    dU[p] = M @ dU[p] + _embedded(dm[p], int(o["placement"]), ctype) @ U
                U = M @ U
            U_all[c], dU_all[c] = U, dU
        res = {"U": U_all, "dU": dU_all, "ov": None, "dov": None}
        if int(K["target_off"]) >= 0:
            V = targets[int(K["target_off"]):int(K["target_off"]) + d * d].reshape(d, d)
            cols = [j for j in range(d) if column_mask >> j & 1]
            res["ov"] = np.einsum("ij,cij->c", np.conj(V[:, cols]), U_all[:, :, cols])
            res["dov"] = np.einsum("ij,cpij->cp", np.conj(V[:, cols]), dU_all[:, :, :, cols])
        out.append(res)
    return out


def unpack(circuits, n_candidates, ov, full):
    """The flat outputs of ``N.compose_circuits`` (host arrays or None) in the shape of :func:`interpret`."""
    out = []
    for K in circuits:
        d, P, C = 2 ** int(K["n_wires"]), int(K["n_params"]), n_candidates
        res = {"U": None, "dU": None, "ov": None, "dov": None}
        if full is not None:
            res["U"] = full[int(K["u_off"]):int(K["u_off"]) + C * d * d].reshape(C, d, d)
            res["dU"] = full[int(K["du_off"]):int(K["du_off"]) + C * P * d * d].reshape(C, P, d, d)
        if ov is not None and int(K["target_off"]) >= 0:
            res["ov"] = ov[int(K["ov_off"]):int(K["ov_off"]) + C]
            res["dov"] = ov[int(K["dov_off"]):int(K["dov_off"]) + C * P].reshape(C, P)
        out.append(res)
    return out


# the structs of include/qmle_sv.h as numpy records
CIRCUIT = np.dtype([("op_begin", "<i4"), ("op_end", "<i4"), ("n_wires", "<i4"), ("n_params", "<i4"),
                    ("target_off", "<i8"), ("ov_off", "<i8"), ("dov_off", "<i8"), ("u_off", "<i8"), ("du_off", "<i8")])
OP = np.dtype([("kind", "<i4"), ("placement", "<i4"), ("mat_off", "<i8"), ("mat_stride", "<i8"),
               ("term_begin", "<i4"), ("term_end", "<i4")])
TERM = np.dtype([("slot", "<i4"), ("param", "<i4"), ("coef_off", "<i8")])
N_SOLVES = 7


def _unitary(rng, k, batch=None):
    shape = (k, k) if batch is None else (batch, k, k)
    q, _ = np.linalg.qr(rng.normal(size=shape) + 1j * rng.normal(size=shape))
    return q


def hand_built_tables(C, P, seed=11):
    """One launch that mixes a 1-wire and a 2-wire circuit with every kind and placement ([1, 0] included), shared and
    per-candidate matrices, two terms of one op on one parameter, one parameter in three ops, one parameter in none
    (the only one of circuit 2; with P >= 3 also the last one of circuits 0 and 1), and a 2-wire circuit without
    target and without ops.  -> the keyword arguments of :func:`interpret` plus ``ov_len`` / ``full_len``."""
    rng = np.random.default_rng(seed)
    mats, coefs, targets, rows, ops, terms, circuits = [], [], [], [], [], [], []
    used = max(1, P - 1) if P >= 3 else P  # parameters that may occur (the last one of P >= 3 occurs in none)

    def mat(k, per_candidate):
        m = _unitary(rng, k, C if per_candidate else None)
        mats.append(m.reshape(-1))
        return sum(len(x) for x in mats) - m.size, (k * k if per_candidate else 0)

    def coef(shared_value=None):
        coefs.append(np.full(C, shared_value) if shared_value is not None else rng.normal(size=C))
        return C * (len(coefs) - 1)

    def op(kind, placement, per_candidate=False, params=()):
        t0 = len(terms)
        for p in params:
            terms.append((int(rng.integers(0, 5)) if kind == PULSE else 0, p, coef(1.0 if len(terms) % 3 == 0 else None)))
        if kind == PULSE:
            at, stride = C * len(rows), 0
            rows.append(rng.integers(0, N_SOLVES, size=C))
        else:
            at, stride = mat(2 if placement <= 2 else 4, per_candidate)
        ops.append((kind, placement, at, stride, t0, len(terms)))

    def circuit(n_wires, b, with_target=True):
        d = 2 ** n_wires
        t = -1
        if with_target:
            t = sum(len(x) for x in targets)
            targets.append(_unitary(rng, d).reshape(-1))
        circuits.append((b, len(ops), n_wires, P, t, 0, 0, 0, 0))

    some = lambda: int(rng.integers(0, used))  # noqa: E731
    # circuit 0: one wire; parameter 0 in three ops, two terms on parameter (1 % used) in one op
    b = len(ops)
    op(CONST, 0)
    op(PULSE, 0, params=(0, 1 % used, 1 % used))
    op(ROT_X, 0, params=(0,))
    op(ROT_Y, 0, per_candidate=True, params=(some(),))
    op(CONST, 0, per_candidate=True)
    op(ROT_Z, 0, per_candidate=True, params=(0, some()))
    op(PULSE, 0, params=(some(),))
    circuit(1, b)
    # circuit 1: two wires, every placement
    b = len(ops)
    op(PULSE, 1, params=(0, some()))
    op(CONST, 3)
    op(PULSE, 2, params=(some(), some(), some()))
    op(CPHASE, 3, per_candidate=True, params=(0,))
    op(CONST, 4, per_candidate=True)
    op(ROT_Z, 1, per_candidate=True, params=(some(),))
    op(ROT_X, 2, params=(some(),))
    op(CPHASE, 4, params=(some(), 0))
    op(CONST, 1)
    op(ROT_Y, 2, params=(some(),))
    op(CONST, 2, per_candidate=True)
    op(CONST, 4)
    circuit(2, b)
    # circuit 2: one wire, no op has a term: every derivative column is zero
    b = len(ops)
    op(CONST, 0)
    op(PULSE, 0)
    circuit(1, b)
    # circuit 3: two wires, neither target nor ops
    circuit(2, len(ops), with_target=False)
    ov_len = full_len = 0
    out = []
    for b, e, n, p, t, *_ in circuits:
        d = 2 ** n
        out.append((b, e, n, p, t, ov_len if t >= 0 else -1, ov_len + C if t >= 0 else -1, full_len,
                    full_len + C * d * d))
        ov_len += C * (1 + p) if t >= 0 else 0
        full_len += C * (1 + p) * d * d
    jac = rng.normal(size=(N_SOLVES, 6, 2, 2)) + 1j * rng.normal(size=(N_SOLVES, 6, 2, 2))
    jac[:, 0] = _unitary(rng, 2, N_SOLVES)
    return dict(circuits=np.array(out, dtype=CIRCUIT), ops=np.array(ops, dtype=OP), terms=np.array(terms, dtype=TERM),
                rows=np.concatenate(rows).astype(np.int32), n_candidates=C, mats=np.concatenate(mats),
                coefs=np.concatenate(coefs), targets=np.concatenate(targets), jac=jac), ov_len, full_len


def single_candidate(tables, c):
    """The tables of :func:`hand_built_tables` cut down to candidate ``c`` alone -> (tables, ov_len, full_len)."""
    C = tables["n_candidates"]
    ops, terms, circuits = tables["ops"].copy(), tables["terms"].copy(), tables["circuits"].copy()
    for o in ops:
        if o["kind"] == PULSE:
            o["mat_off"] //= C
        else:
            o["mat_off"] += c * o["mat_stride"]
            o["mat_stride"] = 0
    terms["coef_off"] //= C
    ov_len = full_len = 0
    for K in circuits:
        d, P = 2 ** int(K["n_wires"]), int(K["n_params"])
        if K["target_off"] >= 0:
            K["ov_off"], K["dov_off"] = ov_len, ov_len + 1
            ov_len += 1 + P
        K["u_off"], K["du_off"] = full_len, full_len + d * d
        full_len += (1 + P) * d * d
    return dict(tables, circuits=circuits, ops=ops, terms=terms, rows=tables["rows"].reshape(-1, C)[:, c].copy(),
                n_candidates=1, coefs=tables["coefs"].reshape(-1, C)[:, c].copy()), ov_len, full_len


def column_scale(ref):
    """``max(1, max |reference column|)`` per column of ``[..., d, d]``: the scale of the project's 1e-12 bar."""
    return np.maximum(1.0, np.max(np.abs(ref), axis=-2, keepdims=True)).astype(np.float64)
