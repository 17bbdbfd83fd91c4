"""The status codes of the eight adjoint-sweep entry points for calls that are refused on the host; no GPU.

Every row of ``ROWS`` is one bad call, made through each of twelve columns: per precision the Z sweep, the Pauli
sweep, and both cotangent forms (offsets and indices) with a Z seed and with a Pauli seed.  The device pointers point
nowhere and are never read.  The expected codes are literals, recorded from the library before the sweeps were folded
into shared helpers: a call that is bad in two ways must keep the code of the check that came first, and the two
precisions order their checks differently (complex64: the plans' flags, the cotangent request, then -- behind the
first device call -- workspace, wire masks, slots; complex128: wire masks, slots and marks term by term, the
cotangent request, the workspace, and only then the device).  Where the first device call comes before the deciding
check, a machine without a GPU answers ``HIP``; ``test_gpu_adjoint_status`` repeats those rows where there is one.
"""
import ctypes as C

import pytest

from qml_essentials_amd import _native as N
from qml_essentials_amd import adjoint
from qml_essentials_amd.simulation import LoweredTape, get_plan
from tests.test_abi_cpu import he_layer_ops
from tests.test_matrix_cotangent2_reference_cpu import _tape

INVALID, WIRE, WORKSPACE, UNSUPPORTED, SLOT = -1, -4, -7, -10, -11
P, NULL = C.c_void_p(0x1000), C.c_void_p(None)
COLUMNS = [(prec, entry, seed) for prec in ("", "_f64")
           for entry, seed in (("gradient", "z"), ("gradient", "pauli"), ("cotangent_at", "z"),
                               ("cotangent_at", "pauli"), ("cotangent", "z"), ("cotangent", "pauli"))]


class Setup:
    """n = 3, batch 1; forward tape RX, MAT2_ROW, MAT1_ROW, MAT2, so the reverse tape is MAT2, MAT1_ROW, MAT2_ROW, RX"""

    def __init__(self):
        low, _u2, _u1 = _tape(1)
        rev_ops, terms, *_ = adjoint.build_reverse(low, adjoint._op_blobs(low), [True] + [False] * (low.n_slots - 1),
                                                   [False] * 4, two_wire=True)
        self.terms = terms
        self.fwd, self.rev = get_plan(low), get_plan(LoweredTape(rev_ops, 3), adjoint.REV_FLAGS)
        # other plans: four qubits; one whose neighbouring rotations merged (three source gates, fewer operators);
        # the from-zero variant of a tiled plan (24 qubits, 96 gates), which only qmle_run_batch may execute
        ops4, slots4 = he_layer_ops(4)
        self.four = N.Plan(ops4, 4, slots4, flags=adjoint.REV_FLAGS)
        self.merged = N.Plan([("RX", [0], [0], -1), ("RY", [0], [1], -1), ("RZ", [1], [2], -1)], 3, 3)
        ops24, slots24 = he_layer_ops(24)
        self.top = N.Plan(ops24, 24, slots24, flags=N.PLAN_NO_SPARSE | N.PLAN_NO_ABSORB)
        self.zero_run = self.top.executed("expval")
        assert self.zero_run.describe()["zero_run"] is True

    def call(self, column, **f):
        """One call of `column` with the faults `f` (see ROWS) worked into otherwise valid arguments."""
        prec, entry, seed = column
        L = N.lib()
        fwd, rev = f.get("fwd", self.fwd), f.get("rev", self.rev)
        if f.get("plans") is not None:
            fwd = rev = getattr(self, f["plans"])
        n_terms = {"merged": 3, "zero_run": 96}.get(f.get("plans"), len(self.terms)) + f.get("n_terms_off", 0)
        terms = list(self.terms) + [(-1, 0, 0, 0, 0, 0.0, -1)] * max(0, n_terms - len(self.terms))
        for r, change in f.get("terms", {}).items():  # {reverse op: {field index: value}}
            t = list(terms[r])
            for k, v in change.items():
                t[k] = v
            terms[r] = tuple(t)
        arr = N._adjoint_term_array(terms)
        masks = (C.c_uint32 * 1)(f.get("wire_mask", 1))
        oarr = N.pauli_term_array(f.get("obs_terms", [(1.0, 1, 2, 0)]))
        n_ot, n_obs = f.get("n_obs_terms", 1), f.get("n_obs", 1)
        batch = f.get("batch", 1)
        head = [fwd._h if fwd else None, rev._h if rev else None, f.get("angles_fwd", P), f.get("angles_rev", P), batch,
                f.get("weights", P)]
        tail = [arr if f.get("have_terms", True) else None, n_terms, f.get("grad", P), f.get("n_grad_slots", 1)]
        wsp = f.get("ws", P)
        if entry == "gradient":
            name, wsname = ("gradient", "") if seed == "z" else ("gradient_pauli", "pauli_")
            wsq = getattr(L, "qmle_adjoint_%sworkspace_bytes%s" % (wsname, prec))
            need = wsq(self.fwd._h, self.rev._h, 1) if seed == "z" else wsq(self.fwd._h, self.rev._h, 1, 1, 1)
            obs = [masks if f.get("have_seed", True) else None, n_obs] if seed == "z" else \
                [oarr if f.get("have_seed", True) else None, n_ot, n_obs]
            req = []
        else:
            name = entry
            wsq = getattr(L, "qmle_adjoint_cotangent_at_workspace_bytes" + prec)
            # (the index form serves one-wire gates only and sizes its partial sums for them)
            need = wsq(self.fwd._h, self.rev._h, 1, 1 if seed == "pauli" else 0, 1, int(entry == "cotangent_at"))
            both = f.get("both_seeds", False)
            obs = [masks if (seed == "z" or both) and f.get("have_seed", True) else None,
                   oarr if (seed == "pauli" or both) and f.get("have_seed", True) else None, n_ot, n_obs]
            if entry == "cotangent_at":
                off = f.get("cot_off", [0, 32, 40, -1])
                req = [(C.c_int32 * max(1, len(off)))(*off) if off is not None else None, f.get("cot_stride", 72)]
            else:
                idx = f.get("mat_out", [-1, 0, -1, -1])
                req = [(C.c_int32 * max(1, len(idx)))(*idx) if idx is not None else None, f.get("n_mat", 1)]
            req.append(f.get("d_cot", P))
        ws_bytes = C.c_size_t(need + f.get("ws_bytes_off", 1 << 20))
        fn = getattr(L, "qmle_adjoint_%s%s" % (name, prec))
        return fn(*head, *obs, *tail, *req, wsp, ws_bytes, NULL)


@pytest.fixture(scope="module")
def setup():
    return Setup()


MARKS, SLOT_F = 6, 0  # fields of a term: (out_slot, x_wires, z_wires, proj_wires, n_y, coef, marks_off)
ROT = dict(cot_off=[-1, -1, -1, 0], mat_out=[-1, -1, -1, 0])  # a cotangent flag on the rotation
PAST = dict(cot_off=[0, 65, -1, -1], mat_out=[-1, 1, -1, -1])  # a block past the row / an index past the count
# The codes of a row, in the order of COLUMNS; `_`: the column is not called, because this fault is none for it or
# is decided behind its first device call (recorded without a GPU: QMLE_ERR_HIP there)
I, W, K, U, S, _ = INVALID, WIRE, WORKSPACE, UNSUPPORTED, SLOT, None
ROWS = [
    ("no forward plan", dict(fwd=None), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("no reverse plan", dict(rev=None), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("plans of 4 and 3 qubits", dict(fwd="four"), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("batch 0", dict(batch=0), (I, I, I, I, I, I, I, I, I, I, I, I)),
    # (two states per sample pass one launch's grid in complex64; the complex128 workspace is then too small)
    ("batch 32768", dict(batch=32768), (I, I, I, I, I, I, K, I, I, I, I, I)),
    ("no weights", dict(weights=NULL), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("no seed", dict(have_seed=False), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("both seeds", dict(both_seeds=True), (_, _, I, I, I, I, _, _, I, I, I, I)),
    ("no observable", dict(n_obs=0), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("33 Z observables", dict(n_obs=33), (I, _, I, _, I, _, I, _, I, _, I, _)),
    ("no Pauli term", dict(n_obs_terms=0), (_, I, _, I, _, I, _, I, _, I, _, I)),
    ("a Pauli term on wire 3", dict(obs_terms=[(1.0, 8, 0, 0)]), (_, W, _, W, _, W, _, W, _, W, _, W)),
    ("a Pauli term for observable 1 of 1", dict(obs_terms=[(1.0, 1, 0, 1)]), (_, I, _, I, _, I, _, I, _, I, _, I)),
    ("no terms", dict(have_terms=False), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("one term too few", dict(n_terms_off=-1), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("no gradient", dict(grad=NULL), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("no gradient slot", dict(n_grad_slots=0), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("no workspace", dict(ws=NULL), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("no forward angles", dict(angles_fwd=NULL), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("no reverse angles", dict(angles_rev=NULL), (I, I, I, I, I, I, I, I, I, I, I, I)),
    # (as both plans, with one term per gate; the index form then flags a rotation.  The complex128 sweep walks the
    # lowered operators and asks only that each has one source gate)
    ("a plan compiled for runs from zero", dict(plans="zero_run"), (U, I, I, I, U, U, I, I, I, I, U, U)),
    ("a merged reverse plan", dict(plans="merged"), (I, I, I, I, U, U, I, I, I, I, U, U)),
    ("marks beyond the constants", dict(terms={3: {MARKS: 1 << 20}}), (_, _, _, _, _, _, I, I, I, I, I, I)),
    ("slot 1 of 1", dict(terms={3: {SLOT_F: 1}}), (_, _, _, _, _, _, S, S, S, S, S, S)),
    ("wire mask 0", dict(wire_mask=0), (_, _, _, _, _, _, W, _, W, _, W, _)),
    ("wire mask on wire 3", dict(wire_mask=8), (_, _, _, _, _, _, W, _, W, _, W, _)),
    # (the complex64 query adds the 256 bytes that aligning may take, so its sweep still has enough)
    ("workspace one byte short", dict(ws_bytes_off=-1), (_, I, I, I, I, I, K, I, I, I, I, I)),
    ("workspace one byte short, unaligned", dict(ws_bytes_off=-1, ws=C.c_void_p(0x1001)),
     (_, I, I, I, I, I, K, I, I, I, I, I)),
    ("no offsets / indices", dict(cot_off=None, mat_out=None), (_, _, I, I, I, I, _, _, I, I, I, I)),
    ("no cotangent buffer", dict(d_cot=NULL), (_, _, I, I, I, I, _, _, I, I, I, I)),
    ("stride / count 0", dict(cot_stride=0, n_mat=0), (_, _, I, I, I, I, _, _, I, I, I, I)),
    ("a flag on the rotation", ROT, (_, _, U, U, U, U, _, _, U, U, U, U)),
    ("a two-wire flag", dict(cot_off=[0, -1, -1, -1], mat_out=[0, -1, -1, -1]), (_, _, _, _, U, U, _, _, _, _, U, U)),
    ("a block past the row / an index past the count", PAST, (_, _, S, S, S, S, _, _, S, S, S, S)),
    ("overlapping blocks", dict(cot_off=[0, 31, -1, -1]), (_, _, S, S, _, _, _, _, S, S, _, _)),
    # pairs of faults that the two precisions meet in a different order
    ("from-zero plan and one term too few", dict(plans="zero_run", n_terms_off=-1), (I, I, I, I, I, I, I, I, I, I, I, I)),
    ("from-zero plan and wire mask 0", dict(plans="zero_run", wire_mask=0), (U, I, I, I, U, U, I, I, I, I, U, U)),
    ("merged plan and wire mask 0", dict(plans="merged", wire_mask=0), (I, I, I, I, U, U, I, I, I, I, U, U)),
    ("wire mask 0 and a flag on the rotation", dict(wire_mask=0, **ROT), (_, _, U, U, U, U, W, _, W, U, U, U)),
    ("slot 1 of 1 and a flag on the rotation", dict(terms={3: {SLOT_F: 1}}, **ROT),
     (_, _, U, U, U, U, S, S, S, S, U, U)),
    ("marks beyond the constants and a flag on the rotation", dict(terms={3: {MARKS: 1 << 20}}, **ROT),
     (_, _, U, U, U, U, I, I, I, I, U, U)),
    ("wire mask 0 and workspace short", dict(wire_mask=0, ws_bytes_off=-1), (_, I, I, I, I, I, W, I, I, I, I, I)),
    ("wire mask 0 and slot 1 of 1", dict(wire_mask=0, terms={3: {SLOT_F: 1}}), (_, _, _, _, _, _, W, S, W, S, W, S)),
    ("marks on gate 2, then slot on gate 3", dict(terms={2: {SLOT_F: 0, MARKS: 1 << 20}, 3: {SLOT_F: 1}}),
     (_, _, _, _, _, _, I, I, I, I, I, I)),
    ("slot on gate 2, then marks on gate 3", dict(terms={2: {SLOT_F: 1}, 3: {MARKS: 1 << 20}}),
     (_, _, _, _, _, _, S, S, S, S, S, S)),
    ("slot 1 of 1 and workspace short", dict(terms={3: {SLOT_F: 1}}, ws_bytes_off=-1),
     (_, I, I, I, I, I, S, I, I, I, I, I)),
    ("a block past the row and workspace short", dict(ws_bytes_off=-1, **PAST), (_, I, I, I, S, S, K, I, I, I, S, S)),
]


def _codes(setup, faults, columns, want):
    f = dict(faults)
    if isinstance(f.get("fwd"), str):
        f["fwd"] = getattr(setup, f["fwd"])
    return tuple(setup.call(col, **f) if w is not _ else _ for col, w in zip(columns, want))


@pytest.mark.parametrize("name,faults,want", ROWS, ids=[r[0] for r in ROWS])
def test_every_entry_point_answers_a_bad_call_with_its_recorded_code(setup, name, faults, want):
    assert len(want) == len(COLUMNS) and any(w is not _ for w in want)
    got = _codes(setup, faults, COLUMNS, want)
    print(name, got)
    assert got == want


# What the complex64 sweep decides behind its first device call, with one: the six complex64 columns.  Every call
# made here is refused before a launch (the wire mask is a fault of the Z seeds alone: the Pauli columns stay out);
# "workspace short" takes off the 256 bytes of slack as well, and every other entry point than the Z sweep has
# compared the size with its own query before.
GPU_ROWS = [
    ("workspace 257 bytes short", dict(ws_bytes_off=-257), (K, I, I, I, I, I)),
    ("wire mask on wire 3", dict(wire_mask=8), (W, _, W, _, W, _)),
    ("slot 1 of 1", dict(terms={3: {SLOT_F: 1}}), (S, S, S, S, S, S)),
    ("wire mask 0 and slot 1 of 1", dict(wire_mask=0, terms={3: {SLOT_F: 1}}), (W, S, W, S, W, S)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,faults,want", GPU_ROWS, ids=[r[0] for r in GPU_ROWS])
def test_gpu_adjoint_status(setup, name, faults, want):
    """n = 3, batch 1: the refusals are decided on the host, so no kernel runs and the pointers are never read."""
    got = _codes(setup, faults, COLUMNS[:6], want)
    print(name, got)
    assert got == want


