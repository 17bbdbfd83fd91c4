"""Circuit container + batch dispatcher -- the drop-in boundary of this build.

API mirror of ``qml_essentials/script.py``: ``Script(f, n_qubits)`` and
``Script.execute(type, obs, args=..., kwargs=..., in_axes=..., shots, key)``
(:137-219) with the batched path of ``_execute_batched`` (:399-553).  Where the
reference builds ``jit(vmap(single_execute))``, this class records the circuit
once with :class:`batching.Batched` arguments and hands the tape + angle table to
``libqmle_sv``.  Drawing (``script.py:555-627``) is out of scope.
"""
from __future__ import annotations

import weakref
from typing import Any, Callable, List, Optional, Tuple

import numpy as np

from . import _native as N
from . import distributed, memory, pulses, simulation
from .batching import Batched, to_numpy
from .operations import (MAX_PAULI_WIRES, KrausChannel, Operation, PauliRot, is_wide_matrix_gate, pauli_terms,
                         z_parity_mask)
from .tape import batch_context, recording
from .utils import PRNGKey


class NotAffine(Exception):
    """A gate angle is not an affine function of the device-resident arguments."""


class CompiledCall:
    """One traced circuit whose gate angles are affine in its device-resident arguments.

    Counterpart of the reference's cached ``jit(vmap(...))`` executable
    (``script.py:272-329,469-553``): tracing happens once on a two-row probe; afterwards a
    call is three kernels' worth of work on the GPU -- ``qmle_build_angles`` (angle table
    from the resident ``params`` / ``inputs`` tensors), the plan's passes, the measurement --
    and nothing per sample on the host.
    """

    _holder = None  # weak reference to the call that keeps a workspace (_run_kept)

    def __init__(self, script: "Script", type: str, obs, args: tuple, leaf_ids: Tuple[int, ...],
                 kwargs: dict, upload: bool = True):
        """``upload=False``: the host half only -- the plan and the affine map (``_map``, ``_const``, ``_period``)
        without their device arrays; such a call cannot run (it needs no GPU: the tests read the map from it)."""
        self.type, self.obs = type, list(obs)
        rng = np.random.default_rng(12345)
        probes, wrapped = {}, list(args)
        for k in leaf_ids:  # args[k]: one host row of the device tensor, per-sample shape
            row = np.asarray(args[k], dtype=np.float64)
            pr = np.stack([row, row + rng.uniform(0.1, 1.0, row.shape)])
            probes[k] = pr
            wrapped[k] = Batched.leaf(pr, k)
        tape = script._record_for_engine(*wrapped, **kwargs)
        self.n_qubits = script._n_qubits or simulation.infer_n_qubits(tape, obs)
        # A tape with noise channels runs on vec(rho), a pure "state" of the doubled register
        # (simulation.doubled_tape): the same plan / angle-map machinery, measured as a density matrix.
        # Channels on 3 or 4 wires (applied Kraus operator by Kraus operator) keep the recorded path.
        self.density = any(isinstance(o, KrausChannel) for o in tape)
        n_reg = self.n_qubits
        if self.density:
            if type == "state" or self.n_qubits > simulation.MAX_DENSITY_QUBITS:
                raise NotAffine("noisy tape")  # (the recorded path raises the reference's messages)
            tape = simulation.doubled_tape(tape, self.n_qubits)
            if any(isinstance(it, (simulation._WideChannel, simulation._WideGate)) for it in tape):
                raise NotAffine("wide channel")  # (and wide gates: neither is an operator of a plan)
            n_reg = 2 * self.n_qubits
        self.n_register = n_reg
        low = simulation.LoweredTape(tape, n_reg)
        self.plan = simulation.get_plan(low)
        self.n_slots = low.n_slots
        values = np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (2,))
                           for v in low.values], axis=1) if low.values else np.zeros((2, 0))
        ptr, arg, idx, coef, const = [0], [], [], [], []
        slot = 0
        order = {k: i for i, k in enumerate(leaf_ids)}
        for op_ in tape:
            if op_.lower(n_reg) is None:
                continue
            tans = op_.parameter_tangents
            for j in range(len(op_.lower(n_reg)[2])):  # one slot per lowered parameter
                t = tans[j] if j < len(tans) else []
                if t is None:
                    raise NotAffine(op_.name)
                c0 = values[0, slot]
                c1 = values[1, slot]
                for lid, flat, cf in t:
                    cf = np.broadcast_to(np.asarray(cf, dtype=np.float64), (2,))
                    if abs(cf[0] - cf[1]) > 1e-12 * max(1.0, abs(cf[0])):
                        raise NotAffine(op_.name)
                    arg.append(order[lid]); idx.append(int(flat)); coef.append(float(cf[0]))
                    c0 -= cf[0] * probes[lid][0].reshape(-1)[flat]
                    c1 -= cf[0] * probes[lid][1].reshape(-1)[flat]
                if abs(c0 - c1) > 1e-9 * max(1.0, abs(c0), abs(values[0, slot])):
                    raise NotAffine(op_.name)
                const.append(c0)
                ptr.append(len(arg))
                slot += 1
        self.leaf_ids = leaf_ids
        self._low, self._map = low, (ptr, arg, idx, coef)   # host copies for the adjoint path
        # rotation angles wrap at 4 pi (the gates depend on angle / 2); a DIAG_ALL scale does not
        self._const, self._period = const, [4.0 * np.pi if per else 0.0 for per in low.ops_periodic]
        self._leaf_sizes = {order[k]: int(np.prod(np.shape(args[k]))) for k in leaf_ids}
        self._adj = None
        self._kept = None  # (key, workspace, token, True) of the latest run worth keeping (_run_kept)
        if not upload:
            return
        import torch

        dev = torch.device("cuda", torch.cuda.current_device())
        i32 = lambda v: torch.tensor(v if len(v) else [0], dtype=torch.int32, device=dev)
        f32 = lambda v: torch.tensor(v if len(v) else [0.0], dtype=torch.float32, device=dev)
        self.d_ptr, self.d_arg, self.d_idx = i32(ptr), i32(arg), i32(idx)
        self.d_coef, self.d_const = f32(coef), f32(const)
        self.d_period = torch.tensor(self._period or [0.0], dtype=torch.float64, device=dev)

    def _run_kept(self, batch: int, kind: str, n_obs: int, run):
        """``run(workspace, token) -> (out, workspace, token)`` on the workspace this call keeps.

        One ``(workspace tensor, token)`` pair is kept, for the latest ``(batch, measurement, n_obs)`` on the current
        stream, and only when the executed plan reports that run's chunk loop as ``"free"`` or ``"alone"``: the runs
        whose workspace slots stay zeroed, so that the next call fills nothing (``qmle_run_batch_w``).  Every other run
        leaves nothing behind and allocates as before.  Only one call per process holds a pair at a time.  The pair goes when the key
        changes (before the new run allocates), when the autotuner re-schedules the plan (``Plan.run`` then answers with
        a workspace and token of its own) and on any exception."""
        # only <Z> out of a tiled plan's last pass can leave zeroed slots behind: everything else runs as it always
        # did, without a token (the analysis loops are bound by the host's time per call)
        if kind != "expval":
            return run(None, None)
        tiled = self.__dict__.get("_z_tiled")
        if tiled is None:
            tiled = self._z_tiled = not self.plan.executed("expval").stats()["whole_state_lds"]
        if not tiled:
            return run(None, None)
        import torch

        key = (batch, kind, n_obs, torch._C._cuda_getCurrentRawStream(torch.cuda.current_device()))
        kept, self._kept = self._kept, None
        ws, tok, free = (kept[1], kept[2], kept[3]) if kept is not None and kept[0] == key else (None, 0, None)
        del kept
        out, ws_used, tok = run(ws, tok)
        if tok and (free is None or ws_used is not ws):  # (a token of 0: the run left nothing to keep)
            free = self.plan.executed(kind).describe()["stages"][-1].get("chunk_loop_last_run") in ("free", "alone")
        if tok and free:
            # one kept workspace per process: the call that held the last one lets go of it
            last = CompiledCall._holder() if CompiledCall._holder is not None else None
            if last is not None and last is not self:
                last._kept = None
            CompiledCall._holder = weakref.ref(self)
            self._kept = (key, ws_used, tok, True)
        return out

    def run(self, leaves, divs, mods, batch: int, batch_offset: int = 0, meas: Optional[str] = None,
            shots: Optional[int] = None, key=None):
        """leaves: contiguous float32 CUDA tensors [rows_k, ...] in ``leaf_ids`` order.  ``meas``
        overrides the call's measurement with another one of the same circuit ("mw": Meyer-Wallach
        out of the producing pass, for a call compiled for "state").  ``shots``: "probs" / "expval"
        are estimated from that many draws of the exact probabilities (row b on the Philox stream
        ``(key, batch_offset + b)``, ``simulation.sample_shots``)."""
        if shots is not None and meas is None and self.type in ("probs", "expval"):
            probs = self.run(leaves, divs, mods, batch, batch_offset, meas="probs")
            return simulation.sample_shots(probs, self.n_qubits, self.type, self.obs, shots, key, batch_offset)
        strides = [t[0].numel() if t.shape[0] else 0 for t in leaves]
        if self.density:
            if meas not in (None, self.type, "probs"):
                raise NotImplementedError(f"measurement {meas!r} of a noisy circuit")
            if self.n_slots:
                am = getattr(self, "_amap", None)
                if am is None:
                    am = self._amap = N.AngleMapArgs(len(self.leaf_ids), self.d_ptr, self.d_arg, self.d_idx,
                                                     self.d_coef, self.d_const, self.d_period)
                rho = self.plan.run_map(am.set(leaves, strides, divs, mods, batch_offset), batch, "state", ())
            else:
                import torch
                rho = self.plan.run(torch.zeros((batch, 0), dtype=torch.float32, device=self.d_const.device), "state")
            return simulation.measure_density_vec(rho, self.n_qubits, meas or self.type, self.obs)
        kind = meas if meas is not None and meas != self.type else self.type
        arg = ()
        if kind == "expval":
            how, arg = self._measure()
            if how != "z":
                kind = None
        if kind is not None and self.n_slots:
            # one native call: angle table (scratch) + the batch -- no host time between the two launches
            am = getattr(self, "_amap", None)
            if am is None:
                am = self._amap = N.AngleMapArgs(len(self.leaf_ids), self.d_ptr, self.d_arg, self.d_idx, self.d_coef,
                                                 self.d_const, self.d_period)
            amap = am.set(leaves, strides, divs, mods, batch_offset)
            return self._run_kept(batch, kind, len(arg), lambda ws, tok: self.plan.run_map(
                amap, batch, kind, arg, workspace=ws, token=tok))
        angles = N.build_angles(leaves, strides, divs, mods, self.d_ptr, self.d_arg, self.d_idx,
                                self.d_coef, self.d_const, self.n_slots, batch, batch_offset,
                                d_period=self.d_period)
        if self.n_slots == 0:
            import torch
            angles = torch.zeros((batch, 0), dtype=torch.float32, device=self.d_const.device)
        if meas is not None and meas != self.type:
            return self.plan.run(angles, meas)
        if self.type == "expval":
            how, arg = self._measure()
            if how == "z":
                return self._run_kept(batch, "expval", len(arg), lambda ws, tok: self.plan.run(
                    angles, "expval", arg, workspace=ws, token=tok))
            if how == "parity":
                return self._run_kept(batch, "expval", -len(arg), lambda ws, tok: self.plan.run_parity(
                    angles, arg, workspace=ws, token=tok))
            states = self.plan.run(angles, "state")
            if how == "pauli":
                return N.expval_pauli(states, arg, len(self.obs))
            return simulation._general_expval(states, self.n_qubits, self.obs)
        return self.plan.run(angles, self.type)

    def _measure(self):
        """How the observables are measured (fixed per compiled call): ("z", wires) for plain Z's,
        ("parity", wire groups) for Z-parities, ("pauli", term list) when every observable is a sum of
        Pauli words (one pass over the stored states), ("general", None) otherwise."""
        m = getattr(self, "_meas", None)
        if m is None:
            masks = [z_parity_mask(o) for o in self.obs]
            if self.obs and all(k is not None and len(k) == 1 for k in masks):
                m = ("z", [k[0] for k in masks])
            elif self.obs and all(k is not None for k in masks) and len(masks) <= 32:
                m = ("parity", masks)
            else:
                terms = simulation.pauli_term_list(self.obs, self.n_qubits)
                m = ("pauli", terms) if terms is not None else ("general", None)
            self._meas = m
        return m

    def _adjoint_setup(self):
        """Reverse tape, generator terms and the chain-rule matrices -- built once.  The compiled path keeps the
        angle-only form of ``adjoint.build_reverse`` (every reverse column is minus a forward column), which refuses
        per-sample matrices: a tape with a ``MAT1_ROW`` raises ``AdjointUnsupported`` here, and pulse leaves that
        depend on an argument do not compile in the first place."""
        import torch

        from . import adjoint

        ptr, arg, idx, coef = self._map
        low = self._low
        want = [ptr[s_ + 1] > ptr[s_] for s_ in range(low.n_slots)]
        rev_ops, terms, rev_src = adjoint.build_reverse(low, adjoint._op_blobs(low), want)
        rev = simulation.LoweredTape(rev_ops, self.n_qubits)
        dev = self.d_const.device
        mats = []
        for k in range(len(self.leaf_ids)):  # angle_s = const_s + sum_t coef_t * leaf[arg_t][idx_t]
            m = np.zeros((max(1, low.n_slots), self._leaf_sizes[k]), dtype=np.float32)
            for s_ in range(low.n_slots):
                for t in range(ptr[s_], ptr[s_ + 1]):
                    if arg[t] == k:
                        m[s_, idx[t]] += coef[t]
            mats.append(torch.from_numpy(m).to(dev))
        self._adj = dict(
            rev=rev,
            terms=adjoint.patch_marks(rev, terms),
            perm=torch.tensor(rev_src if rev_src else [0], dtype=torch.int64, device=dev),
            n_rev_slots=rev.n_slots, mats=mats)
        return self._adj

    def vjp(self, leaves, divs, mods, batch: int, weights):
        """Adjoint gradient of ``sum_k weights[b, k] <obs_k>_b`` with respect to the device
        leaves -> list of CUDA tensors shaped like ``leaves`` (a leaf shared by the whole batch
        receives the sum over the batch).  Angle table, forward pass, backward sweep and the
        chain rule all stay on the GPU."""
        import torch

        if self.density:
            raise NotImplementedError("adjoint differentiation of a noisy circuit")
        masks = [z_parity_mask(o) for o in self.obs]
        if self.type != "expval" or not self.obs or any(m is None for m in masks):
            raise NotImplementedError("adjoint differentiation needs Z / Z-parity observables")
        adj = self._adj or self._adjoint_setup()
        strides = [int(np.prod(t.shape[1:], dtype=np.int64)) for t in leaves]
        angles = N.build_angles(leaves, strides, divs, mods, self.d_ptr, self.d_arg, self.d_idx,
                                self.d_coef, self.d_const, self.n_slots, batch, 0,
                                d_period=self.d_period)
        if adj["n_rev_slots"]:
            rev_angles = (-angles.index_select(1, adj["perm"])).contiguous()
        else:
            rev_angles = torch.zeros((batch, 1), dtype=torch.float32, device=angles.device)
        from . import adjoint

        d = adjoint.run_sweep(self.plan, adj["rev"], angles, rev_angles, weights, masks,
                              adj["terms"], max(1, self.n_slots))               # [B, n_slots]
        out = []
        for k, leaf in enumerate(leaves):
            g = d @ adj["mats"][k]                                               # [B, leaf size]
            rows = int(leaf.shape[0])
            if rows == 1:
                g = g.sum(dim=0, keepdim=True)
            elif not (divs[k] == 1 and rows == batch):
                row = (torch.arange(batch, device=g.device) // int(divs[k])) % int(mods[k])
                g = torch.zeros((rows, g.shape[1]), dtype=g.dtype, device=g.device).index_add_(0, row, g)
            out.append(g.reshape(tuple(leaf.shape)))
        return out


class Script:
    """Wraps a circuit function ``f(*args, **kwargs)`` that instantiates operations."""

    def __init__(self, f: Callable[..., None], n_qubits: Optional[int] = None) -> None:
        self.f = f
        self._n_qubits = n_qubits
        self._compiled: dict = {}  # structure key -> CompiledCall (device-resident path)

    def compiled(self, key, type: str, obs, args: tuple, leaf_ids: Tuple[int, ...],
                 kwargs: Optional[dict] = None) -> CompiledCall:
        """Fetch / build the :class:`CompiledCall` for ``key`` (raises :class:`NotAffine`)."""
        cc = self._compiled.get(key)
        if cc is None:
            if callable(args):  # probe values are only needed to build the call
                args = args()
            cc = CompiledCall(self, type, obs, args, leaf_ids, kwargs or {})
            if len(self._compiled) > 64:
                self._compiled.pop(next(iter(self._compiled)))
            self._compiled[key] = cc
        return cc

    def _record(self, *args, **kwargs) -> List[Operation]:
        with recording() as tape:
            self.f(*args, **kwargs)
        return tape

    def _record_for_engine(self, *args, **kwargs) -> List[Operation]:
        """The recorded tape as the engine takes it.  A Pauli rotation whose word has no opcode goes as an explicit
        matrix if it is batch-constant on at most two wires; on more wires, or with a per-sample angle, it is replaced
        by its decomposition (one- and two-wire gates, the angle and its tangents on one RZ)."""
        tape = self._record(*args, **kwargs)

        def wide(o) -> bool:
            return (isinstance(o, PauliRot) and o.pauli_word not in PauliRot._NATIVE_WORDS
                    and (len(o.wires) > 2 or np.ndim(o.theta) > 0))

        if not any(wide(o) for o in tape):
            return tape
        out: List[Operation] = []
        for o in tape:
            out.extend(o.decompose() if wide(o) else [o])
        return out

    @staticmethod
    def _batch_size(args: tuple, in_axes: Tuple) -> int:
        for a, ax in zip(args, in_axes):
            if ax is not None:
                return int(np.shape(a)[ax])
        return 1

    def execute(self, type: str = "expval", obs: Optional[List[Operation]] = None, *,
                args: tuple = (), kwargs: Optional[dict] = None, in_axes: Optional[Tuple] = None,
                shots: Optional[int] = None, key=None, as_tensor: bool = False, wide_gates: bool = False):
        """Execute the circuit; with ``in_axes`` the result has a leading batch axis.  ``wide_gates=True`` serves a
        noisy tape that holds explicit matrices on three or four wires (``op.prod(...)``, ``A @ B``,
        ``Operation(wires, matrix)``, evolved unitaries of 8x8 / 16x16 Hamiltonians) beside Kraus channels: every
        measurement type but ``"state"``, shots, complex64 and x64, un-batched and with ``in_axes``.  Without it such a
        tape is refused; on a noise-free tape the keyword changes nothing.  Still refused with it: matrices and
        channels on five or more wires, ``vjp(noisy=True)`` through wide gates or wide channels, ``gradient``."""
        from .tape import captured_call

        with captured_call(lambda: dict(kind="script", script=self, type=type, obs=obs, args=args,
                                        kwargs=kwargs, in_axes=in_axes, shots=shots)) as cap:
            cap["result"] = self._execute(type, obs, args, kwargs, in_axes, shots, key, as_tensor, wide_gates)
        return cap["result"]

    def _execute(self, type, obs, args, kwargs, in_axes, shots, key, as_tensor, wide_gates=False):
        obs = [] if obs is None else obs
        kwargs = {} if kwargs is None else kwargs
        if shots is not None and key is None:
            key = PRNGKey(0)  # script.py:189-190
        if in_axes is not None:
            return self._execute_batched(type, obs, args, kwargs, in_axes, shots, key, as_tensor, wide_gates)
        tape = self._record_for_engine(*[to_numpy(a) for a in args], **kwargs)
        pulses.resolve(tape)  # every pulse leaf of the tape in one launch
        n_qubits = self._n_qubits or simulation.infer_n_qubits(tape, obs)
        res = simulation.simulate_and_measure(
            tape, n_qubits, type, obs, simulation.uses_density(tape, type), shots=shots, key=key,
            as_tensor=as_tensor, **({"wide_gates": True} if wide_gates else {}),
        )
        if simulation._tape_batch(tape) == 1:
            res = res[0]
        return res

    def _execute_batched(self, type, obs, args, kwargs, in_axes, shots=None, key=None,
                         as_tensor: bool = False, wide_gates: bool = False):
        if len(in_axes) != len(args):
            raise ValueError(
                f"in_axes has {len(in_axes)} entries but args has {len(args)}. "
                "Provide one in_axes entry per positional argument."
            )
        args = tuple(to_numpy(a) for a in args)
        batch_size = self._batch_size(args, in_axes)
        n_obs = len(obs)

        def run(start: int, end: int):
            wrapped = []
            for a, ax in zip(args, in_axes):
                if ax is None or a is None:
                    wrapped.append(a)
                else:
                    wrapped.append(Batched(np.moveaxis(np.asarray(a), ax, 0)[start:end]))
            with batch_context(end - start):
                tape = self._record_for_engine(*wrapped, **kwargs)
            pulses.resolve(tape)
            n_qubits = self._n_qubits or simulation.infer_n_qubits(tape, obs)
            return simulation.simulate_and_measure(
                tape, n_qubits, type, obs, simulation.uses_density(tape, type), shots=shots,
                key=key, batch=end - start, as_tensor=as_tensor, row_offset=start,
                **({"wide_gates": True} if wide_gates else {}),  # (said only where asked for: the call is as it was otherwise)
            ), n_qubits, len(tape)

        # memory-aware chunking needs n_qubits / n_ops: probe with one sample's structure
        n_qubits = self._n_qubits
        n_ops = 1
        use_density = False
        if n_qubits is None or kwargs.get("noise_params"):
            probe = [a if ax is None or a is None else Batched(np.moveaxis(np.asarray(a), ax, 0)[:1])
                     for a, ax in zip(args, in_axes)]
            tape = self._record_for_engine(*probe, **kwargs)
            n_qubits = n_qubits or simulation.infer_n_qubits(tape, obs)
            n_ops = len(tape)
            use_density = any(isinstance(o, KrausChannel) for o in tape)
        # multi-GPU: this rank simulates one contiguous block of the batch; one
        # all-gather returns the full result everywhere (script.py:443-453)
        lo, hi, sharded = distributed.my_block(batch_size, *args)
        local = hi - lo
        from .utils import x64_enabled

        x64 = x64_enabled() and shots is None
        # (complex128 mode: 16-byte amplitudes, and observables the engine does not measure itself --
        # anything but Z / Z-parities -- keep every sample's state for the contraction)
        general = x64 and type == "expval" and any(z_parity_mask(o) is None for o in (obs or []))
        chunk = memory.compute_chunk_size(n_qubits, local, type, use_density, n_obs, n_ops=n_ops,
                                          x64=x64, general_obs=general)
        if chunk >= local:
            res = run(lo, hi)[0]
        else:
            res = memory.execute_chunked(lambda s, e: run(lo + s, lo + e)[0], local, chunk)
        if sharded:
            res = distributed.all_gather_rows(res, batch_size)
        return res

    # ------------------------------------------------------------------ gradients
    _SHIFT_RULES = {
        # (shift, coefficient) terms:  df/dtheta = sum_k coef_k * f(theta + shift_k)
        "two": ((np.pi / 2, 0.5), (-np.pi / 2, -0.5)),
        # controlled rotations (generator spectrum {0, +-1/2}): four-term rule
        "four": ((np.pi / 2, (np.sqrt(2) + 1) / (4 * np.sqrt(2))),
                 (-np.pi / 2, -(np.sqrt(2) + 1) / (4 * np.sqrt(2))),
                 (3 * np.pi / 2, -(np.sqrt(2) - 1) / (4 * np.sqrt(2))),
                 (-3 * np.pi / 2, (np.sqrt(2) - 1) / (4 * np.sqrt(2)))),
    }

    def _trace_for_gradient(self, obs, args, kwargs, in_axes, argnums, skip_channels: bool = False,
                            mat_ops: Optional[list] = None, through_evolve: bool = False, wide_gates: bool = False):
        """Record the tape with the ``argnums`` arguments as differentiable leaves.  Returns
        ``(tape, lowered tape, n_qubits, B, slots, leaf_shapes, batched)`` where ``slots`` lists
        ``(angle slot, shift rule, tangent terms)`` for every angle that depends on a leaf.
        ``skip_channels``: noise channels stay on the returned tape but take no part in the lowered
        tape and the slot numbering (the mixed-state QFI).
        ``mat_ops``: a list that receives ``(index in the lowered tape's ops, operation)`` for every matrix gate
        whose matrix depends on a leaf through a known Jacobian (pulse leaves: ``wants_matrix_cotangent``); such a
        gate is then solved with its sensitivities here and does not count as "non-linear".  Only a caller that
        asks the sweep for matrix cotangents passes it (:meth:`vjp`).
        ``through_evolve``: the tape is recorded inside ``evolution.gradient_trace()``, so that evolved gates whose
        arguments depend on a leaf are solved with their Jacobian and want a matrix cotangent too.
        ``wide_gates``: a tape that holds explicit matrices on 3 or 4 wires is not lowered as a whole (the lowered
        tape comes back as None); slots keep tape order, wide gates holding none, and ``mat_ops`` then receives
        ``(index of the tape entry, operation)``."""
        kwargs = {} if kwargs is None else kwargs
        args = tuple(to_numpy(a) for a in args)
        batched = in_axes is not None
        if in_axes is None:
            in_axes = (None,) * len(args)
        if len(in_axes) != len(args):
            raise ValueError(
                f"in_axes has {len(in_axes)} entries but args has {len(args)}. "
                "Provide one in_axes entry per positional argument."
            )
        B = self._batch_size(args, in_axes) if batched else 1
        wrapped, leaf_shapes = [], {}
        for k, (a, ax) in enumerate(zip(args, in_axes)):
            if a is None or not hasattr(a, "shape"):
                wrapped.append(a)
                continue
            arr = np.asarray(a, dtype=np.float64)
            data = np.moveaxis(arr, ax, 0) if ax is not None else np.broadcast_to(arr, (B,) + arr.shape)
            if k in argnums:
                wrapped.append(Batched.leaf(np.array(data), k))
                leaf_shapes[k] = data.shape[1:]
            elif ax is not None:
                wrapped.append(Batched(data, []))  # batched, but a constant for this gradient
            else:
                wrapped.append(a)
        if through_evolve:
            from . import evolution

            with evolution.gradient_trace(wide=wide_gates):
                tape = self._record_for_engine(*wrapped, **kwargs)
        else:
            tape = self._record_for_engine(*wrapped, **kwargs)
        n_qubits = self._n_qubits or simulation.infer_n_qubits(tape, obs)
        gates = [o for o in tape if not isinstance(o, KrausChannel)] if skip_channels else tape
        if mat_ops is not None:  # U and dU/d(arguments) of every pulse leaf that depends on a leaf: one launch group
            pulses.resolve_for_gradient(gates)
        segmented = wide_gates and any(is_wide_matrix_gate(o) for o in gates)
        if segmented and any(isinstance(o, KrausChannel) for o in gates):
            from .adjoint import AdjointUnsupported

            raise AdjointUnsupported("adjoint differentiation of noisy circuits (explicit matrices on 3 or 4 wires are "
                                     "not available on noisy tapes)")
        low = None if segmented else simulation.LoweredTape(gates, n_qubits)

        # differentiable slots: (slot, rule, tangent terms)
        slots, s, k_op = [], 0, -1
        for k_entry, op_ in enumerate(gates):
            if segmented and is_wide_matrix_gate(op_):  # no angle slot; a cotangent where its Jacobian is known
                if mat_ops is not None and getattr(op_, "wants_matrix_cotangent", False):
                    mat_ops.append((k_entry, op_))
                elif op_.__dict__.get("_matrix_tangent", []) is None:
                    raise NotImplementedError(
                        f"{op_.name}: parameter is a non-linear function of the arguments; "
                        "cannot apply the chain rule")
                continue
            lowered = op_.lower(n_qubits)
            if lowered is None:
                continue
            k_op += 1
            if mat_ops is not None and getattr(op_, "wants_matrix_cotangent", False):
                mat_ops.append((k_entry if segmented else k_op, op_))  # (its lowered parameters are matrix entries, not angles)
                s += len(lowered[2])
                continue
            tans = op_.parameter_tangents
            for j in range(len(lowered[2])):  # one angle slot per lowered parameter
                t = tans[j] if j < len(tans) else []
                if t is None:
                    raise NotImplementedError(
                        f"{op_.name}: parameter is a non-linear function of the arguments; "
                        "cannot apply the chain rule")
                if t:
                    slots.append((s, op_._shift_rule, t, op_.name))
                s += 1
        return tape, low, n_qubits, B, slots, leaf_shapes, batched

    def vjp(self, obs: List[Operation], cotangent, *, args: tuple = (),
            kwargs: Optional[dict] = None, in_axes: Optional[Tuple] = None,
            argnums: Tuple[int, ...] = (0,), pauli_seed: bool = False, through_evolve: bool = False,
            wide_gates: bool = False, noisy: bool = False):
        """Gradient of ``sum_k cotangent[b, k] * <obs_k>_b`` with respect to the array arguments
        ``argnums`` by ADJOINT differentiation: one backward sweep for all angles
        (:mod:`adjoint`).  ``obs``: at most 32 Z / Z-parity observables seed the sweep from their wire masks.
        With ``pauli_seed=True`` any other list that is a sum of Pauli words (``simulation.pauli_term_list``:
        PauliX / PauliY, products, Hermitian matrices on up to ``MAX_PAULI_WIRES`` wires) seeds it with
        ``lambda = H psi`` from the Pauli-word kernels; more than 32 Z parities take that seed in any case, as
        x = 0 words.  Without the flag an observable with an X / Y / Hermitian factor raises
        ``AdjointUnsupported`` as it always did (callers rely on that refusal to fall back to the parameter-shift
        Jacobian).  A batched matrix, a parametrised observable and a wider Hermitian have no term list:
        ``AdjointUnsupported`` either way, as for noisy circuits.  ``cotangent`` has shape
        ``(B, n_obs)`` (``(n_obs,)`` without ``in_axes``).  Returns one array per ``argnums``
        entry of shape ``(B, *arg_shape)`` (no ``B`` axis without ``in_axes``).  A ``cotangent`` with a
        leading axis of K cotangents, ``(K, B, n_obs)``, is served by one trace and one sweep over K * B
        states and returns ``(K, B, *arg_shape)`` (a Jacobian: K = n_obs one-hot rows).

        Pulse leaves (:class:`pulses.PulseRotation`) whose arguments depend on a leaf are differentiated too: they
        are solved with their sensitivities (``pulses.resolve_for_gradient``), the same sweep returns their matrix
        cotangents ``G`` beside the angle gradients, and ``2 Re sum_ac G[a][c] J[slot][a][c] coef`` is added for every
        ``(leaf, slot, index, coef)`` of ``leaf_jacobian_terms()``.  An argument the recorder lost track of raises
        ``NotImplementedError``; an evolved gate (a per-sample matrix that is no pulse leaf) on the tape raises
        ``AdjointUnsupported``, as before -- unless ``through_evolve=True``.

        ``through_evolve=True`` differentiates through ``Hermitian.evolve()`` / ``ParametrizedHamiltonian.evolve()``
        gates in the same ONE sweep: the tape is recorded inside ``evolution.gradient_trace()``, every evolved gate
        whose time, interval ends or coefficient parameters depend on a leaf is solved with the exact Jacobian of its
        grid (``qmle_evolve_magnus_jac``) and contributes ``2 Re sum_ac G[a][c] dU[a][c]/d(leaf element)`` like a pulse
        leaf; an evolved gate that is a constant for this gradient is just inverted by the sweep.  Evolved gates on one
        and on two wires are served (2x2 and 4x4 cotangents from ``adjoint.adjoint_slot_and_matrices_gradient``);
        Hamiltonians on more wires are refused by ``evolve()`` itself.

        ``wide_gates=True`` serves tapes that hold explicit matrices on three or four wires (``op.prod(...)``,
        ``A @ B``, a user's ``Operation(wires, matrix)``, evolved unitaries of 8x8 and 16x16 Hamiltonians, one matrix
        for all samples or one per sample): the sweep runs segment by segment between them
        (``adjoint.segmented_gradient``) and gives the gradient of every ordinary angle, of pulse leaves and of one-
        and two-wire evolved gates on the same tape, for Z and Pauli seeds and K-stacked cotangents, in complex64 and
        x64.  A wide gate that is a constant of the gradient is simply inverted.  With ``through_evolve=True`` as
        well, a STATIC evolved gate on three or four wires, ``Hermitian(H, wires).evolve()(t)`` with ``t`` depending
        on a leaf, is differentiated from ``dU/dt = -i H U``.  Still refused: a ``ParametrizedHamiltonian`` on three
        or four wires that depends on a leaf (the wide solver has no Jacobian form), matrices on five or more wires,
        noisy tapes; ``Script.gradient``, compiled calls, ``Model`` and the torch bridge do not take such tapes.
        Without the keyword every refusal is what it was.

        ``noisy=True`` serves a tape that holds Kraus channels on one and two wires: the sweep runs over vec(rho) with
        the forward states kept (``adjoint.density_gradient``, ``qmle_adjoint_density``) and gives the gradient of
        every ordinary angle for Z / parity seeds, ``pauli_seed=True``, ``(K, B, n_obs)`` cotangents (K cotangents
        share one forward run) and ``in_axes``, in complex64 and x64.  Refused with ``AdjointUnsupported``, naming the
        operation: channels on three or four wires, full-register diagonal encodings, per-sample matrices (pulse and
        evolved gates, also with ``through_evolve``), explicit matrices on three or four wires; derivatives with
        respect to noise strengths are not formed.  A tape without a channel takes the pure-state sweep as before, and
        without the keyword a noisy tape is refused as it always was."""
        from . import adjoint

        if not obs:
            raise adjoint.AdjointUnsupported("adjoint differentiation needs at least one observable")
        masks = [z_parity_mask(o) for o in obs]
        if any(m is None for m in masks) and not pauli_seed:
            kinds = sorted({type(o).__name__ for o, m in zip(obs, masks) if m is None})
            raise adjoint.AdjointUnsupported(
                "adjoint differentiation needs Z / Z-parity observables; pauli_seed=True seeds the sweep with "
                "H psi for sums of Pauli words (got " + ", ".join(kinds) + ")")
        mat_ops: list = []
        tape, low, n_qubits, B, slots, leaf_shapes, batched = self._trace_for_gradient(
            obs, args, kwargs, in_axes, argnums, mat_ops=mat_ops, through_evolve=through_evolve, wide_gates=wide_gates,
            **({"skip_channels": True} if noisy else {}))
        on_rho = any(isinstance(o, KrausChannel) for o in tape)  # (noisy=True: the sweep over vec(rho))
        if on_rho and not noisy:
            raise adjoint.AdjointUnsupported("adjoint differentiation of noisy circuits")
        if on_rho and mat_ops:
            raise adjoint.AdjointUnsupported(f"adjoint differentiation of noisy circuits: {mat_ops[0][1].name} (a pulse "
                                             "or evolved gate: a per-sample matrix) is not served")
        segmented = low is None  # (wide_gates=True and a wide gate on the tape: the sweep segment by segment)
        for o in tape:  # without through_evolve evolved gates stay out of scope: nothing differentiates one
            if segmented and is_wide_matrix_gate(o):  # (constant or carrying its Jacobian: _trace_for_gradient)
                continue
            m = getattr(o, "_matrix", None)
            per_sample = not isinstance(o, pulses.PulseRotation) and getattr(o, "_native", None) is None \
                and isinstance(m, np.ndarray) and m.ndim == 3
            if per_sample and not through_evolve:
                raise adjoint.AdjointUnsupported(
                    f"no adjoint rule for {o.name} (MAT1_ROW / MAT2_ROW): a per-sample matrix that is not a pulse "
                    "leaf (an evolved unitary) has no generator and no Jacobian the sweep could differentiate")
        # the chain rule of every pulse leaf, before any device work (an argument the recorder lost track of raises)
        mat_terms = [o.leaf_jacobian_terms() for _k, o in mat_ops]
        obs_terms = None
        if any(m is None for m in masks) or len(obs) > 32:  # not the Z seed: the observables as weighted Pauli words
            masks, obs_terms = None, simulation.pauli_term_list(obs, n_qubits)
            if obs_terms is None:
                kinds = sorted({type(o).__name__ for o in obs if pauli_terms(o) is None})
                raise adjoint.AdjointUnsupported(
                    "adjoint differentiation needs observables that are sums of Pauli words: "
                    + (", ".join(kinds) + " has none (a batched matrix, a parametrised observable or more than "
                       f"{MAX_PAULI_WIRES} wires)" if kinds else "the term list exceeds the library's limits"))
        from .utils import x64_enabled

        x64 = x64_enabled()  # complex128 sweep, float64 tables (jax.grad with jax_enable_x64, test_jaqsi.py:57)
        w = np.asarray(cotangent, dtype=np.float64 if x64 else np.float32)
        K = int(w.size // (B * len(obs)))  # K > 1: ``cotangent`` is (K, B, n_obs) -- K cotangents, ONE trace and sweep
        stacked = K > 1 or w.ndim == 3
        w = w.reshape(K * B, len(obs))
        want = [False] * (adjoint.tape_slot_count(tape, n_qubits) if segmented else low.n_slots)
        for s_, _rule, _t, _name in slots:
            want[s_] = True
        grads = {k: np.zeros((K, B) + tuple(shp)) for k, shp in leaf_shapes.items()}
        # a per-sample matrix that nothing is asked of (an evolved gate that is a constant for this gradient) still
        # needs the form of the reverse tape that inverts it
        row_ops = not segmented and through_evolve and any(name in ("MAT1_ROW", "MAT2_ROW")
                                                           for name, _w, _s, _off in low.ops)
        if on_rho:
            if slots:
                d = adjoint.density_gradient(tape, n_qubits, B, masks, w, want, x64=x64, obs_terms=obs_terms)
        elif segmented:
            cots = []
            if mat_ops or slots:  # one [K * B, d, d] per flagged tape entry, d = 2, 4, 8 or 16
                want_mat = [False] * len(tape)
                for k_entry, _o in mat_ops:
                    want_mat[k_entry] = True
                d, cots = adjoint.segmented_gradient(tape, n_qubits, B, masks, w, want, want_mat, x64=x64,
                                                     obs_terms=obs_terms)
        elif mat_ops or (row_ops and slots):  # angle slots and matrix cotangents from ONE sweep
            want_mat = [False] * len(low.ops)
            for k_op, _o in mat_ops:
                want_mat[k_op] = True
            if through_evolve:  # one [K * B, d, d] per flagged op, d = 2 or 4
                d, cots = adjoint.adjoint_slot_and_matrices_gradient(low, n_qubits, B, masks, w, want, want_mat,
                                                                     x64=x64, obs_terms=obs_terms)
            else:
                d, cot = adjoint.adjoint_slot_and_matrix_gradient(low, n_qubits, B, masks, w, want, want_mat, x64=x64,
                                                                  obs_terms=obs_terms)  # [K * B, n_mat, 2, 2]
                cots = [cot[:, m] for m in range(len(mat_ops))]
        elif slots:
            d = adjoint.adjoint_slot_gradient(low, n_qubits, B, masks, w, want, x64=x64,
                                              obs_terms=obs_terms)  # [K * B, n_slots]
        for m, ((_k, o), terms) in enumerate(zip(mat_ops, mat_terms)):
            jac = np.asarray(o.jacobian, dtype=np.complex128)  # [B or 1, D, d, d]: D = 5 for a pulse leaf
            jac = jac.reshape(jac.shape[0], jac.shape[1], -1)
            g_m = np.asarray(cots[m], dtype=np.complex128).reshape(K, B, jac.shape[-1])  # (the op's own d * d)
            # dC/d(slot) = 2 Re sum_ac G[a][c] dU[a][c]/d(slot)  -> [K, B, D]
            per_slot = 2.0 * np.real(np.einsum("kbe,bse->kbs", g_m,
                                               np.broadcast_to(jac, (B,) + jac.shape[1:])))
            for lid, slot, flat, coef in terms:
                g = grads[lid].reshape(K, B, -1)
                g[:, :, int(flat)] += per_slot[:, :, slot] * np.asarray(coef, dtype=np.float64).reshape(1, -1)
        if slots:
            d = d.reshape(K, B, -1)
            for s_, _rule, tangent, _name in slots:
                for lid, flat, coef in tangent:  # gate angles are scalars: one leaf element each
                    g = grads[lid].reshape(K, B, -1)
                    g[:, :, int(flat)] += d[:, :, s_] * np.asarray(coef, dtype=np.float64).reshape(1, B)
        if not stacked:
            grads = {k: g[0] for k, g in grads.items()}
            return tuple(grads[k] if batched else grads[k][0] for k in argnums)
        return tuple(grads[k] if batched else grads[k][:, 0] for k in argnums)

    def gradient(self, obs: List[Operation], *, args: tuple = (), kwargs: Optional[dict] = None,
                 in_axes: Optional[Tuple] = None, argnums: Tuple[int, ...] = (0,)):
        """Jacobian of ``execute(type="expval", obs=obs, ...)`` with respect to the array
        arguments ``argnums`` by the parameter-shift rule (exact, no finite differences).

        What ``jax.grad`` through ``Script.execute`` provides in the reference
        (``tests/test_jaqsi.py:131-141,764-786``), done the way this engine is good at:
        every shifted circuit is one more row of the batch, so one engine call evaluates
        all ``2 x (#rotation gates)`` (4 per controlled rotation) shifted copies of every
        sample.  Gate angles may be sums / products of the arguments (``inputs * enc_params``);
        the chain rule uses the tangents tracked by :class:`batching.Batched`.

        Returns a tuple with one array per entry of ``argnums`` of shape
        ``(B, n_obs, *arg_shape)`` (``arg_shape`` without its batch axis); ``B = 1`` and the
        axis is dropped when ``in_axes`` is None.
        """
        tape, low, n_qubits, B, slots, leaf_shapes, batched = self._trace_for_gradient(
            obs, args, kwargs, in_axes, argnums)
        from .utils import x64_enabled

        base = low.angle_table(B, dtype=np.float64) if x64_enabled() else low.angle_table(B).astype(np.float64)
        grads = {k: np.zeros((B, len(obs)) + tuple(shp)) for k, shp in leaf_shapes.items()}
        if slots:
            rows = []
            for slot, rule_name, _t, op_name in slots:
                if rule_name is None:
                    raise NotImplementedError(f"{op_name} has no parameter-shift rule")
                for shift, _c in self._SHIFT_RULES[rule_name]:
                    t = base.copy()
                    t[:, slot] += shift
                    rows.append(t)
            if x64_enabled():  # shifted circuits on the complex128 engine, gate by gate like simulate()
                table = np.concatenate(rows, axis=0)
                plan = simulation.get_plan(low, (simulation.PLAN_FLAGS or 0) | N.PLAN_NO_MERGE)
            else:
                table = np.concatenate(rows, axis=0).astype(np.float32)
                plan = simulation.get_plan(low)
            vals = simulation.run_expval_table(plan, table, obs, n_qubits)  # (rows*B, n_obs)
            vals = vals.reshape(-1, B, len(obs))
            r = 0
            for slot, rule_name, tangent, _op_name in slots:
                d = np.zeros((B, len(obs)))
                for _shift, coef in self._SHIFT_RULES[rule_name]:
                    d += coef * vals[r]
                    r += 1
                for lid, flat, coef in tangent:
                    g = grads[lid].reshape(B, len(obs), -1)
                    g[:, :, flat] += d * np.asarray(coef).reshape(-1, 1)
        out = tuple(grads[k] if batched else grads[k][0] for k in argnums)
        return out

    # ------------------------------------------------------------------ quantum geometric tensor
    # State rules (operators, not expectation values):  dU/dtheta = sum_k coef_k U(theta + shift_k).
    # Pauli rotations exp(-i theta G / 2), G^2 = I (RX/RY/RZ, Rot's factors, PauliRot, RXX/RYY/RZZ/RZX):
    # U(theta + pi) = -sin(theta/2) - i cos(theta/2) G = 2 dU/dtheta.  Controlled rotations: the target block
    # is a Pauli rotation and U(theta - pi) flips its sign only there.  CPhase: diag(.., e^{i phi}).
    _STATE_RULES = {
        "pauli": ((np.pi, 0.5),),
        "controlled": ((np.pi, 0.25), (-np.pi, -0.25)),
        "phase": ((np.pi / 2, 0.5), (-np.pi / 2, -0.5)),
    }

    @staticmethod
    def state_rule(op_name: str, shift_rule: Optional[str]) -> str:
        """Which entry of ``_STATE_RULES`` differentiates the state through a gate (``NotImplementedError``
        for a gate without one)."""
        if op_name in ("ControlledPhaseShift", "CPhase"):
            return "phase"
        if shift_rule == "four":
            return "controlled"
        if shift_rule == "two":
            return "pauli"
        raise NotImplementedError(f"{op_name}: no state derivative rule (quantum geometric tensor)")

    @staticmethod
    def fold_qgt(coef, gram):
        """``Q = C Gamma C^T - (C Gamma)_{:,0} (C Gamma)_{:,0}^H`` for real ``coef`` ``(B, P, R+1)`` and
        the Gram matrices ``gram`` ``(B, R+1, R+1)`` of the rows (row 0 = the unshifted state), fp64."""
        coef = np.asarray(coef, dtype=np.float64)
        gram = np.asarray(gram, dtype=np.complex128)
        # real products of Re / Im, one point at a time (np.dot: BLAS, where a stacked complex matmul is not)
        cg = np.empty(gram.shape[:1] + coef.shape[1:], dtype=np.complex128)
        m = np.empty(coef.shape[:2] + coef.shape[1:2], dtype=np.complex128)
        for b in range(coef.shape[0]):
            cre, cim = np.dot(coef[b], gram[b].real), np.dot(coef[b], gram[b].imag)
            cg[b] = cre + 1j * cim
            m[b] = np.dot(cre, coef[b].T) + 1j * np.dot(cim, coef[b].T)
        v = cg[:, :, 0]
        return m - v[:, :, None] * np.conj(v)[:, None, :]

    def _qgt_rows(self, tape, low, n_qubits, B, slots, leaf_shapes, argnums, mixed: bool = False):
        """The shifted angle table ``(B, R+1, n_slots)`` (row 0 unshifted) and the fold coefficients
        ``(B, P, R+1)``; ``mixed`` uses the expectation-value rules (they hold for rho itself)."""
        from .utils import x64_enabled

        base = low.angle_table(B, dtype=np.float64) if x64_enabled() else low.angle_table(B).astype(np.float64)
        offsets, P = {}, 0
        for k in argnums:
            offsets[k] = P
            P += int(np.prod(leaf_shapes[k])) if k in leaf_shapes else 0
        shifts, terms = [], []  # per row: (slot, shift); per row: [(column of C, coef (B,))]
        for slot, rule_name, tangent, op_name in slots:
            if mixed:
                if rule_name is None:
                    raise NotImplementedError(f"{op_name} has no parameter-shift rule")
                rule = self._SHIFT_RULES[rule_name]
            else:
                rule = self._STATE_RULES[self.state_rule(op_name, rule_name)]
            for shift, c in rule:
                shifts.append((slot, shift))
                terms.append([(offsets[lid] + int(flat), c * np.broadcast_to(np.asarray(tc, dtype=np.float64),
                                                                          (B,)))
                              for lid, flat, tc in tangent if lid in offsets])
        R1 = len(shifts) + 1
        table = np.repeat(base[:, None, :], R1, axis=1)
        coef = np.zeros((B, P, R1))
        for r, ((slot, shift), tt) in enumerate(zip(shifts, terms), start=1):
            table[:, r, slot] += shift
            for col, c in tt:
                coef[:, col, r] += c
        return table, coef

    def quantum_geometric_tensor(self, *, args: tuple = (), kwargs: Optional[dict] = None,
                                 in_axes: Optional[Tuple] = None, argnums: Tuple[int, ...] = (0,),
                                 row_block: Optional[int] = None):
        """Quantum geometric tensor ``Q_ij = <d_i psi|d_j psi> - <d_i psi|psi><psi|d_j psi>`` of the
        circuit's output state with respect to the flattened ``argnums`` arguments (the order of
        :meth:`gradient`); ``Re Q`` is the Fubini-Study metric, ``4 Re Q`` the quantum Fisher information.

        Every derivative state is a fixed real combination of shifted circuits (``_STATE_RULES``), so one
        engine call runs the unshifted and the shifted rows of every point, ``qmle_gram`` forms their Gram
        matrix ``Gamma = S^H S`` on the device and the fold ``C Gamma C^T`` (``fold_qgt``) runs on the host.
        Noisy (density) tapes return the mixed-state QFI ``/ 4`` as a real tensor (:func:`math._qfi_density`
        on ``d rho`` from the expectation-value shift rules, at most 7 qubits).

        Returns complex ``(B, P, P)`` (no ``B`` axis without ``in_axes``).  ``row_block`` forces the split
        of each point's rows into blocks of that many (the path taken when one point's states exceed
        free HBM, :func:`memory.metric_plan`)."""
        tape, low, n_qubits, B, slots, leaf_shapes, batched = self._trace_for_gradient(
            [], args, kwargs, in_axes, argnums, skip_channels=True)
        if any(isinstance(o, KrausChannel) for o in tape):
            q = self._qfi_mixed(tape, low, n_qubits, B, slots, leaf_shapes, argnums) / 4.0
            return q if batched else q[0]
        from .utils import x64_enabled

        x64 = x64_enabled()
        torch = N.require_gpu()
        table, coef = self._qgt_rows(tape, low, n_qubits, B, slots, leaf_shapes, argnums)
        R1 = table.shape[1]
        if x64:
            plan = simulation.get_plan(low, (simulation.PLAN_FLAGS or 0) | N.PLAN_NO_MERGE)
        else:
            plan = simulation.get_plan(low)

        def states(rows):  # rows of the angle table -> [len(rows), 2^n] states on the device
            rows = np.ascontiguousarray(rows)
            if x64:
                return plan.run64(torch.from_numpy(rows).cuda(), "state")
            return plan.run(torch.from_numpy(rows.astype(np.float32)).cuda(), "state")

        chunk, block = memory.metric_plan(n_qubits, R1, B, x64=x64)
        if row_block is not None:
            block, chunk = max(1, min(int(row_block), R1)), 1 if int(row_block) < R1 else chunk
        gram = np.empty((B, R1, R1), dtype=np.complex128)
        D = 1 << n_qubits
        if block >= R1:
            for b0 in range(0, B, chunk):
                b1 = min(B, b0 + chunk)
                s = states(table[b0:b1].reshape(-1, table.shape[2]))
                gram[b0:b1] = N.to_host(N.gram(s.reshape(b1 - b0, R1, D)))
                del s
        else:
            cuts = list(range(0, R1, block)) + [R1]
            for b in range(B):
                for I in range(len(cuts) - 1):
                    i0, i1 = cuts[I], cuts[I + 1]
                    si = states(table[b, i0:i1]).reshape(1, i1 - i0, D)
                    gram[b, i0:i1, i0:i1] = N.to_host(N.gram(si))[0]
                    for J in range(I + 1, len(cuts) - 1):
                        j0, j1 = cuts[J], cuts[J + 1]
                        sj = states(table[b, j0:j1]).reshape(1, j1 - j0, D)
                        g = N.to_host(N.gram(si, sj))[0]
                        gram[b, i0:i1, j0:j1] = g
                        gram[b, j0:j1, i0:i1] = np.conj(g.T)
                        del sj
                    del si
        q = self.fold_qgt(coef, gram)
        return q if batched else q[0]

    def _qfi_mixed(self, tape, low, n_qubits, B, slots, leaf_shapes, argnums):
        """QFI ``(B, P, P)`` of the output density matrix of a noisy tape: ``rho`` and every shifted
        ``rho`` from one run of the density engine, ``d_i rho = sum_r C_ir rho_r``, then the SLD formula."""
        from . import math as qmath
        from .utils import x64_enabled

        if n_qubits > qmath.MAX_MIXED_QFI_QUBITS:
            raise ValueError(f"the mixed-state QFI is computed on the host from eigh(rho): at most "
                             f"{qmath.MAX_MIXED_QFI_QUBITS} qubits (got {n_qubits})")
        table, coef = self._qgt_rows(tape, low, n_qubits, B, slots, leaf_shapes, argnums, mixed=True)
        R1 = table.shape[1]
        rows = table.reshape(B * R1, -1)  # (b, r) row-major
        # the recorded tape with every angle slot replaced by its column of the shifted table
        shifted, s = [], 0
        import copy

        for op_ in tape:
            lowered = op_.lower(n_qubits) if not isinstance(op_, KrausChannel) else None
            new = copy.copy(op_)
            if lowered is not None:
                if "_tangents" in op_.__dict__:
                    new._tangents = dict(op_._tangents)
                for j in range(len(lowered[2])):
                    new._store_param(op_._param_names[j], Batched(rows[:, s].copy(), []))
                    s += 1
            elif isinstance(op_, KrausChannel):
                for name in getattr(op_, "_param_names", ()):
                    v = getattr(op_, name, None)
                    if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == B:
                        setattr(new, name, np.repeat(v, R1, axis=0))
            shifted.append(new)
        rho = simulation._simulate_mixed(shifted, n_qubits, "density", [], B * R1, x64=x64_enabled())
        rho = np.asarray(N.to_host(rho), dtype=np.complex128).reshape(B, R1, 2**n_qubits, 2**n_qubits)
        out = np.empty((B, coef.shape[1], coef.shape[1]))
        for b in range(B):
            drho = np.einsum("pr,rkl->klp", coef[b], rho[b])
            out[b] = qmath._qfi_density(drho, rho[b, 0])
        return out

    def draw(self, *a, **k):
        raise NotImplementedError("circuit drawing is outside the MI355X hot path")
