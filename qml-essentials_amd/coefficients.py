"""Numerical Fourier coefficients of a model (``Coefficients``, FFT path).

API mirror of ``qml_essentials/coefficients.py:23-237``: ``get_spectrum``,
``_fourier_transform``, ``get_psd``, ``evaluate_Fourier_series``.  The cost is the
batched model evaluation on the input grid (``:130``) -- that is the HIP engine's
job, sharded across ranks by :class:`script.Script`; the FFT of the few thousand
expectation values is done with NumPy on the host.

``FCC`` (Fourier-coefficient correlation, ``coefficients.py:966-1650``) sits downstream:
its cost is again the ``B_I x B_P`` batch of circuit evaluations (grid points x parameter
samples) on the engine; the correlation of the resulting ``(n_freq, n_samples)`` matrix is
small dense linear algebra done here on the host.  ``Datasets`` generates the synthetic
Fourier-series targets the reference trains on (``coefficients.py:1652-1788``).
``FourierTree`` (``coefficients.py:240-963``) is the analytic route: the sine-cosine tree of the canonical
Pauli-Clifford circuit, merged into a DAG on the host and walked with numbers by the HIP kernel ``qmle_fourier_dag``
-- exact coefficients without a sampling grid, for every parameter set of a batch in one launch.
"""
from __future__ import annotations

import functools
import logging
import math
import sys
import warnings
from types import SimpleNamespace
from typing import Any, List, Optional, Tuple, Union

import numpy as np
from scipy.stats import rankdata

from .model import Model
from .operations import PauliWord
from .pauli import PauliCircuit

log = logging.getLogger(__name__)


class Coefficients:
    @classmethod
    def get_spectrum(cls, model: Model, mfs: int = 1, mts: int = 1, shift: bool = False,
                     trim: bool = False, numerical_cap: Optional[float] = -1,
                     **kwargs) -> Tuple[np.ndarray, np.ndarray]:
        """FFT coefficients and their frequencies; ``mfs`` / ``mts`` oversample in
        frequency / time (``coefficients.py:25-106``)."""
        kwargs.setdefault("force_mean", True)
        kwargs.setdefault("execution_type", "expval")
        coeffs, freqs = cls._fourier_transform(model, mfs=mfs, mts=mts, **kwargs)
        imag = float(np.sum(coeffs).imag)
        if not abs(imag) <= 1.0e-6:  # (= np.isclose(imag, 0.0, atol=1e-6), without its 8 us; NaN fails too)
            raise ValueError(f"Spectrum is not real. Imaginary part of coefficients is: {imag}")
        if trim:
            for ax in range(model.n_input_feat):
                if coeffs.shape[ax] % 2 == 0:
                    coeffs = np.delete(coeffs, len(coeffs) // 2, axis=ax)
                    freqs = [np.delete(f, len(f) // 2, axis=ax) for f in freqs]
        if shift:
            coeffs = np.fft.fftshift(coeffs, axes=list(range(model.n_input_feat)))
            freqs = np.fft.fftshift(freqs)
        if numerical_cap is not None and numerical_cap > 0:
            coeffs = np.where(np.abs(coeffs) < numerical_cap, np.zeros_like(coeffs), coeffs)
            if model.n_input_feat == 1:
                alive = coeffs != 0 if coeffs.ndim == 1 else np.any(
                    coeffs != 0, axis=tuple(range(1, coeffs.ndim)))
                coeffs = coeffs[alive]
                freqs = [np.asarray(freqs[0])[alive]]
        if len(freqs) == 1:
            freqs = freqs[0]
        return coeffs, freqs

    @classmethod
    def _fourier_transform(cls, model: Model, mfs: int, mts: int, **kwargs: Any):
        """Sample the model on ``x_k = 2 pi k / N_f`` per feature and FFT
        (``coefficients.py:109-150``; feature 0 is the slowest grid axis)."""
        F = model.n_input_feat
        # the engine returns float32; the (tiny) host FFT runs in double so that it adds no
        # rounding noise of its own to the spectrum.  complex128 mode (utils.enable_x64 /
        # Model(x64=True)): the grid stays float64 too -- a float32-rounded grid point is off by
        # 1e-7 rad, which leaks 1e-8 into the analytically vanishing top-frequency coefficients
        from .utils import x64_enabled

        x64 = x64_enabled() if getattr(model, "x64", None) is None else bool(model.x64)
        # grid, frequencies and the device copy of the grid depend on (degrees, mfs, mts) only: a
        # spectrum is asked for again and again on the same grid, and the ~40 us of numpy calls that
        # build it are a fifth of a 4096-point call
        key = (tuple(mfs * model.degree[i] for i in range(F)), mts, x64)
        hit = cls._PLANS.get(key)
        if hit is None:
            n_freqs = np.array(key[0])
            axes = [np.arange(0, 2 * mts * np.pi, 2 * np.pi / n_freqs[i]) for i in range(F)]
            grid = np.array(np.meshgrid(*axes)).T.reshape(-1, F)
            freqs = [np.fft.fftfreq(int(mts * n_freqs[i]), 1 / n_freqs[i]) for i in range(F)]
            lens = [a.shape[0] for a in axes]
            if len(cls._PLANS) > 32:
                cls._PLANS.clear()
            hit = cls._PLANS[key] = (grid, freqs, lens)
        grid, freqs, lens = hit
        freqs = [f.copy() for f in freqs]  # (callers may edit what they get back)
        grid_dev = None if x64 else cls._device_grid(grid)
        if grid_dev is not None:
            # the grid lives on the GPU (cached per grid): nothing is uploaded per call, and the
            # ONE device -> host copy is the (few thousand) model values.  Their FFT stays on the
            # host in float64: numpy transforms 4096 points in ~25 us, a device FFT costs twice that
            # in launch bookkeeping alone, and numpy's real-input transform is exactly Hermitian
            # (|c_k| == |c_-k| bit for bit, which numerical_cap relies on)
            outputs = model(inputs=grid_dev, **kwargs)
            if hasattr(outputs, "is_cuda"):
                outputs = outputs.cpu().numpy()
        else:
            outputs = model(inputs=grid if x64 else grid.astype(np.float32), **kwargs)
        outputs = np.asarray(outputs, dtype=np.float64).reshape(*lens, -1).squeeze()
        if F == 1 and outputs.ndim >= 1 and outputs.shape[0] == lens[0] > 2:
            return cls._fft_real(outputs), freqs
        coeffs = np.fft.fftn(outputs, axes=list(range(F)))
        return coeffs / math.prod(outputs.shape[0:F]), freqs

    @staticmethod
    def _fft_real(values: np.ndarray) -> np.ndarray:
        """``fft(values, axis=0) / N`` of REAL float64 samples: the half spectrum (``rfft``) and its
        conjugate mirror -- exactly Hermitian by construction and half the work of the complex
        transform (4096 points: 16 us instead of 30 on the bench host)."""
        n = values.shape[0]
        half = np.fft.rfft(values, axis=0, norm="forward")
        out = np.empty((n,) + half.shape[1:], dtype=np.complex128)
        out[:n // 2 + 1] = half
        out[n // 2 + 1:] = np.conj(half[1:(n + 1) // 2][::-1])
        return out

    _GRIDS: dict = {}
    _PLANS: dict = {}  # (n_freqs, mts, x64) -> (host grid, frequency axes, grid lengths)

    @classmethod
    def _device_grid(cls, grid: np.ndarray):
        """float32 CUDA copy of an input grid, cached (a spectrum is usually asked for again and
        again on the same grid); None without a GPU."""
        from .utils import _gpu_present

        if not _gpu_present():
            return None
        import torch

        key = (grid.shape, float(grid[-1].sum()), float(grid[len(grid) // 2].sum()), torch.cuda.current_device())
        hit = cls._GRIDS.get(key)
        if hit is None or (hit[0] is not grid and not np.array_equal(hit[0], grid)):
            if len(cls._GRIDS) > 16:
                cls._GRIDS.clear()
            hit = cls._GRIDS[key] = (grid, torch.from_numpy(grid.astype(np.float32)).cuda())
        return hit[1]

    @classmethod
    def get_psd(cls, coeffs: np.ndarray) -> np.ndarray:
        coeffs = np.asarray(coeffs)
        return (2.0 / (len(coeffs) ** 2)) * (coeffs.real**2 + coeffs.imag**2)

    @classmethod
    def evaluate_Fourier_series(cls, coefficients, frequencies,
                                inputs: Union[np.ndarray, list, float]) -> np.ndarray:
        """sum_k c_k exp(i <w_k, x>) at the given points (``coefficients.py:172-237``)."""
        coefficients = np.asarray(coefficients)

        def flatten(freq_axes):
            freq_axes = [np.asarray(f) for f in freq_axes]
            mesh = np.stack(np.meshgrid(*freq_axes, indexing="ij"), axis=-1)
            ff = mesh.reshape(-1, len(freq_axes))
            return coefficients.reshape(ff.shape[0], *coefficients.shape[len(freq_axes):]), ff

        if isinstance(frequencies, list):
            fc, ff = flatten(frequencies)
        else:
            frequencies = np.asarray(frequencies)
            if frequencies.ndim == 1:
                ff = frequencies[:, None]
                fc = coefficients.reshape(ff.shape[0], *coefficients.shape[1:])
            else:
                n_feat, n_axis = frequencies.shape
                if coefficients.shape[:n_feat] == (n_axis,) * n_feat:
                    fc, ff = flatten(frequencies)
                else:
                    ff = frequencies
                    fc = coefficients.reshape(ff.shape[0], *coefficients.shape[1:])
        x = np.asarray(inputs)
        if x.ndim == 0:
            x = x.reshape(1, 1)
        elif x.ndim == 1:
            if ff.shape[1] == 1:
                x = x[:, None]
            elif x.shape[0] == ff.shape[1]:
                x = x[None, :]
            else:
                x = np.repeat(x[:, None], ff.shape[1], axis=1)
        phases = np.exp(1j * (x @ ff.T))
        return np.squeeze(np.real(np.tensordot(phases, fc, axes=([1], [0]))))


TREE_LAUNCHES = 0  # calls of qmle_fourier_dag since import (one per workspace chunk of an evaluation with evaluate="device")
TREE_WORKSPACE_BYTES = 4 << 30  # default budget of device (or host) memory for the node values of one chunk


class FourierTreeTooLarge(RuntimeError):
    """The merged DAG has more than ``max_nodes`` nodes, the explicit tree more than ``max_leaves`` leaves, or one
    sample's node values do not fit the workspace budget."""


_popcount = int.bit_count if hasattr(int, "bit_count") else (lambda v: bin(v).count("1"))


class FourierTree:
    """Analytic Fourier coefficients of a Pauli-Clifford circuit: the sine-cosine tree of Nemkov et al. (Phys. Rev. A
    108, 032406), API of ``coefficients.py:240-963``.

    The circuit is brought to its canonical form -- Pauli rotations ``exp(-i theta_k P_k / 2)`` behind an evolved
    observable word (:class:`pauli.PauliCircuit`) -- and the observable is pulled through the rotations, last first:
    a rotation that commutes is skipped, one that does not splits the word ``O`` into ``cos(theta) O + i sin(theta)
    P O``.  The reference enumerates every leaf of that binary tree.  Here nodes with the same ``(rotation index,
    bare word)`` are merged -- their values differ by a power of i that moves onto the edge -- which turns the tree
    into a DAG of a few thousand to a million nodes where the tree has up to ``10^20`` leaves.  The DAG is built once
    on the host (:meth:`_ensure_dag`) and evaluated with numbers: on the frequency grid for :meth:`get_spectrum`,
    where an input rotation ``cos / i sin`` is half the sum / difference of two shifts, and on plain numbers for
    :meth:`__call__`.  ``evaluate="device"`` (the default when a GPU is present) walks it in the HIP kernel
    ``qmle_fourier_dag``, every parameter set of a batch in one launch per workspace chunk
    (:data:`TREE_LAUNCHES`); ``evaluate="host"`` is a float64 NumPy interpreter of the same tables.

    Beyond the reference: ``get_spectrum(params=...)`` and ``__call__(params=..., inputs=...)`` take a batch of
    parameter sets (leading axis as after ``initialize_params(repeat=B)``; ``__call__`` also a batch of inputs) and
    return ``(B, n_freq)`` coefficients per root / values shaped like the model's.

    The reference's leaf enumeration survives for ``get_exact_support("tree")`` and the introspection attributes
    ``leaf_arrays``, ``weights_per_root``, ``freqs_per_root``: built lazily on the host, bounded by ``max_leaves``,
    and used by nothing numeric.
    """

    def __init__(self, model: Model, evaluate: Optional[str] = None, max_nodes: int = 1 << 22,
                 max_leaves: int = 1 << 20, workspace_bytes: Optional[int] = None) -> None:
        self._check_evaluate(evaluate)
        self.model = model
        self.n_qubits = model.n_qubits
        if self.n_qubits > 64:
            raise NotImplementedError("FourierTree packs a Pauli word into two 64-bit masks: at most 64 qubits")
        self.evaluate = evaluate
        self.max_nodes = int(max_nodes)
        self.max_leaves = int(max_leaves)
        self.workspace_bytes = workspace_bytes

        # one parameter set and a base input fix the canonical tape: which words appear does not depend on the values
        self._params = self._single_param_set(model.params)
        base_inputs = np.ones(model.n_input_feat)
        operations, observables = self._build_canonical_tape(self._params, base_inputs)
        self.parameters = [np.squeeze(p) for p in PauliCircuit.get_parameters(operations)]
        self.n_params = len(self.parameters)
        self.pauli_words: List[PauliWord] = [PauliWord.from_operation(o, self.n_qubits) for o in operations]
        self.cumulative_xy: List[np.ndarray] = []
        running = np.zeros(self.n_qubits, dtype=bool)
        for w in self.pauli_words:  # X/Y support of rotations 0..k: the light cone of the cut
            running = running | w.xy_mask
            self.cumulative_xy.append(running.copy())
        self.observable_words: List[PauliWord] = [PauliWord.from_operation(o, self.n_qubits) for o in observables]
        self._detect_inputs(base_inputs)
        self._dag = None
        self._structure_built = False

    # ---- recording ------------------------------------------------------------------------------
    @staticmethod
    def _check_evaluate(evaluate) -> None:
        if evaluate not in (None, "host", "device"):
            raise ValueError(f"evaluate must be 'host' or 'device', got {evaluate!r}")

    def _single_param_set(self, params) -> np.ndarray:
        """The tree describes one parameter set: of batched model parameters (after FCC sampling, say) the first is
        used, with a warning."""
        params = np.asarray(params)
        if params.ndim > 2 and params.shape[0] > 1:
            warnings.warn(f"FourierTree supports a single parameter set; using the first of {params.shape[0]} "
                          "batched parameter sets.", UserWarning)
            params = params[0]
        return params

    def _record_canonical(self, params, inputs):
        """Record the model's script once for all of ``params`` ``(B_P, ...)`` x ``inputs`` ``(B_I, d)`` (batched like
        a model call: inputs slowest) and canonicalise the tape.  -> (rotations, observables, B_I, B_P, B), B the number
        of samples of the recording."""
        from .batching import Batched, to_numpy
        from .tape import batch_context

        m = self.model
        params = np.asarray(to_numpy(params), dtype=np.float64)
        if params.ndim == 2:
            params = params[None]
        inputs = m._inputs_validation(inputs)
        zero_inputs = m._zero_inputs
        enc_params = m._enc_params_validation(None)
        inputs, params = m._assimilate_batch(inputs, params)
        B_I, B_P = int(m.batch_shape[0]), int(m.batch_shape[1])
        B = int(np.prod(m.eff_batch_shape))
        if B > 1:
            if B_P > 1:
                params = Batched(params)
            if B_I > 1:
                inputs = Batched(inputs)
        # an all-zero input still records its encoding gates here (the tape keeps its columns); the model's own flag
        # is put back as validation left it
        m._zero_inputs = False
        try:
            with batch_context(B):
                tape = m.script._record(params, inputs, None, None, enc_params)
        finally:
            m._zero_inputs = zero_inputs
        _, obs = m._build_obs()
        rotations, observables = PauliCircuit.from_parameterised_circuit(tape, observables=obs,
                                                                         n_qubits=self.n_qubits)
        return rotations, observables, B_I, B_P, B

    def _build_canonical_tape(self, params, inputs):
        rotations, observables, _, _, _ = self._record_canonical(self._single_param_set(params), inputs)
        return rotations, observables

    def _canonical_angles(self, params, inputs) -> Tuple[np.ndarray, int, int]:
        """The canonical rotation angles ``[B, n_params]`` (float64) of a batch, and ``(B_I, B_P)``."""
        rotations, _, B_I, B_P, B = self._record_canonical(params, inputs)
        cols = PauliCircuit.get_parameters(rotations)
        if hasattr(self, "n_params") and len(cols) != self.n_params:
            raise RuntimeError(f"the recorded circuit has {len(cols)} Pauli rotations, the tree was built for "
                               f"{self.n_params}: the circuit's structure must not depend on its arguments")
        angles = np.empty((B, len(cols)), dtype=np.float64)
        for k, p in enumerate(cols):
            angles[:, k] = np.asarray(p, dtype=np.float64).reshape(-1)
        return angles, B_I, B_P

    def _canonical_parameters(self, inputs) -> np.ndarray:
        return self._canonical_angles(self._params, inputs)[0][0]

    def _detect_inputs(self, base_inputs: np.ndarray) -> None:
        """Find the input-encoding columns from the tape alone.  Every canonical angle is linear in the inputs (an
        encoding angle is ``w x_f``, and Clifford commutation only flips signs), so stepping one feature by 1 and
        differencing the recorded angles gives, per column, the feature it reads and its signed integer scaling.
        Sets ``input_indices`` ``{feature: [columns]}``, ``all_input_indices``, ``input_scaling`` (1 for variational
        columns), ``var_positions`` and ``features``."""
        tol = 1e-6
        d = self.model.n_input_feat
        base = np.asarray(base_inputs, dtype=float)
        p_base = np.array([float(p) for p in self.parameters])
        response = np.zeros((d, self.n_params))
        for f in range(d):
            stepped = base.copy()
            stepped[f] += 1.0
            response[f] = self._canonical_parameters(stepped) - p_base
        input_indices: dict = {}
        all_input_indices: List[int] = []
        scaling = np.ones(self.n_params, dtype=np.int64)
        for k in range(self.n_params):
            feats = np.flatnonzero(np.abs(response[:, k]) > tol)
            if feats.size == 0:
                continue
            if feats.size > 1:
                raise NotImplementedError(
                    f"Rotation {k} depends on multiple input features {feats.tolist()}; the Fourier tree requires "
                    "each encoding rotation to be linear in a single feature.")
            f = int(feats[0])
            omega = float(response[f, k])
            if abs(p_base[k] - omega * base[f]) > tol:
                raise NotImplementedError(
                    f"Rotation {k} has the angle {omega:.4f} x + {p_base[k] - omega * base[f]:.4f}; the Fourier tree "
                    "requires encoding angles without a constant offset.")
            w = int(round(omega))
            if abs(omega - w) > tol:
                warnings.warn(f"Non-integer input scaling {omega:.4f} on rotation {k} (feature {f}); rounding to {w}. "
                              "The Fourier tree supports integer frequency scalings only.", UserWarning)
            input_indices.setdefault(f, []).append(k)
            all_input_indices.append(k)
            scaling[k] = w
        self.input_indices = input_indices
        self.all_input_indices = all_input_indices
        self.input_scaling = scaling
        taken = set(all_input_indices)
        self.var_positions = np.array([k for k in range(self.n_params) if k not in taken], dtype=np.int64)
        self.features = sorted(input_indices)

    # ---- the merged DAG -------------------------------------------------------------------------
    def _packed_words(self):
        """Rotations and observables as ``(x mask, z mask, phase)`` with bit q = qubit q."""
        def pack(word: PauliWord):
            x = sum(int(b) << q for q, b in enumerate(word.x))
            z = sum(int(b) << q for q, b in enumerate(word.z))
            return x, z, word.phase

        return [pack(w) for w in self.pauli_words], [pack(w) for w in self.observable_words]

    def _grid(self):
        """Frequency grid of :meth:`get_spectrum`: per feature axis ``2 sum|w| + 1`` points.  -> (dims, strides,
        flat index of omega = 0)."""
        dims = [2 * int(sum(abs(int(self.input_scaling[k])) for k in self.input_indices[f])) + 1
                for f in self.features]
        strides = [int(np.prod(dims[a + 1:], dtype=np.int64)) for a in range(len(dims))]
        return dims, strides, sum((n - 1) // 2 * s for n, s in zip(dims, strides))

    def _ensure_dag(self):
        """Build the tables of ``qmle_fourier_dag`` (``include/qmle_sv.h``) once.  Recursion from every observable
        word through the rotations, last first: commuting rotations are skipped; a word with an X/Y outside the
        X/Y support of the rotations still ahead can never become diagonal and is cut (the value is 0); nodes are
        memoised on ``(index, x, z)`` packed into one integer; the phase of ``P O`` leaves the node as a power of i
        on the sine edge, the phase of the observable stays with the root.  Beside the node the recursion carries its
        structural frequency support as a bit mask over the grid (the same walk in the boolean semiring: an input
        column moves the union of its children's masks by +-w), and a node whose mask is empty -- no path to a
        diagonal word -- is not created.  All observables share the DAG."""
        if self._dag is not None:
            return self._dag
        from . import _native as N

        paulis, observables = self._packed_words()
        n, K = self.n_qubits, self.n_params
        cum, running = [], 0
        for xp, _, _ in paulis:
            running |= xp
            cum.append(running)
        dims, strides, centre = self._grid()
        axis_of = {f: a for a, f in enumerate(self.features)}
        column_axis = {k: axis_of[f] for f, cols in self.input_indices.items() for k in cols}
        step = [abs(int(self.input_scaling[k])) * strides[column_axis[k]] if k in column_axis else 0 for k in range(K)]
        unit = 1 << centre
        ONE, ZERO = N.FOURIER_ONE, N.FOURIER_ZERO
        level: List[int] = []
        cos_child: List[int] = []
        sin_child: List[int] = []
        power: List[int] = []
        memo: dict = {}
        max_nodes = self.max_nodes

        def visit(idx: int, x: int, z: int):
            while True:
                if idx < 0:
                    return (ONE, unit) if x == 0 else (ZERO, 0)
                if x & ~cum[idx]:
                    return ZERO, 0
                xp, zp, php = paulis[idx]
                if (_popcount(x & zp) + _popcount(z & xp)) & 1:
                    break
                idx -= 1
            key = (((idx << n) | x) << n) | z
            hit = memo.get(key)
            if hit is not None:
                return hit
            c_code, c_mask = visit(idx - 1, x, z)
            s_code, s_mask = visit(idx - 1, x ^ xp, z ^ zp)
            mask = c_mask | s_mask
            if mask == 0:
                res = (ZERO, 0)
            else:
                if step[idx]:
                    mask = (mask << step[idx]) | (mask >> step[idx])
                if len(level) >= max_nodes:
                    raise FourierTreeTooLarge(
                        f"the merged sine-cosine DAG has more than max_nodes = {max_nodes} nodes; pass a larger "
                        "max_nodes to FourierTree if the memory is there")
                res = (len(level), mask)
                level.append(idx)
                cos_child.append(c_code)
                sin_child.append(s_code)
                power.append((php + 2 * _popcount(zp & x)) & 3)  # phase of P O, O the bare word (self.z . other.x)
            memo[key] = res
            return res

        old_limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old_limit, 4 * K + 1000))
        try:
            found = [visit(K - 1, xo, zo) for xo, zo, _ in observables]
        finally:
            sys.setrecursionlimit(old_limit)

        # order the nodes by rotation index: children then sit on lower levels, which is the order of evaluation
        lvl = np.asarray(level, dtype=np.int64)
        order = np.argsort(lvl, kind="stable")
        new_id = np.empty(len(order) + 2, dtype=np.int64)  # (slots -2 and -1 hold the terminal codes)
        new_id[order] = np.arange(len(order))
        new_id[-1], new_id[-2] = ONE, ZERO
        nodes = np.zeros(len(order), dtype=N.FOURIER_NODE)
        nodes["cos_child"] = new_id[np.asarray(cos_child, dtype=np.int64)[order]]
        nodes["sin_child"] = new_id[np.asarray(sin_child, dtype=np.int64)[order]]
        nodes["power"] = np.asarray(power, dtype=np.int64)[order]
        bounds = np.searchsorted(lvl[order], np.arange(K + 1))
        dag = SimpleNamespace(
            nodes=nodes, bounds=bounds, n_nodes=len(nodes), dims=dims, centre=centre,
            roots=np.array([int(new_id[c]) for c, _ in found], dtype=np.int32),
            root_phase=np.array([ph for _, _, ph in observables], dtype=np.int32),
            masks=[m for _, m in found], column_axis=column_axis)
        self._dag = dag
        return dag

    def _levels(self, spectrum: bool) -> np.ndarray:
        """The level table: one level per rotation.  For the spectrum an input column is a SHIFT along its feature's
        axis by its signed scaling; every other column -- and, for a plain evaluation, every column -- is an ANGLE."""
        from . import _native as N

        dag = self._ensure_dag()
        levels = np.zeros(self.n_params, dtype=N.FOURIER_LEVEL)
        levels["node_begin"], levels["node_end"] = dag.bounds[:-1], dag.bounds[1:]
        levels["kind"] = N.FOURIER_KINDS["ANGLE"]
        levels["column"] = np.arange(self.n_params)
        if spectrum:
            for k, axis in dag.column_axis.items():
                levels[k] = (dag.bounds[k], dag.bounds[k + 1], N.FOURIER_KINDS["SHIFT"], 0, axis,
                             int(self.input_scaling[k]))
        return levels

    def _dag_frequencies(self) -> List[np.ndarray]:
        """Per root the structural frequency support, from the masks of :meth:`_ensure_dag`, in the reference's
        layout: sorted, 1-D for at most one feature, ``(n_freq, d)`` otherwise; ``[0]`` for an empty support."""
        dag = self._ensure_dag()
        d = len(dag.dims)
        out = []
        for mask in dag.masks:
            flat = np.array([i for i in range(mask.bit_length()) if (mask >> i) & 1], dtype=np.int64)
            if d == 0 or flat.size == 0:
                freqs = np.zeros((1, max(d, 1)), dtype=np.int64)
            else:
                coords = np.stack(np.unravel_index(flat, dag.dims), axis=1)
                freqs = coords - (np.asarray(dag.dims) - 1) // 2
            out.append(freqs[:, 0] if freqs.shape[1] == 1 else freqs)
        return out

    # ---- numeric evaluation -----------------------------------------------------------------------
    def _resolve_evaluate(self, evaluate) -> str:
        self._check_evaluate(evaluate)
        mode = evaluate or self.evaluate
        if mode is None:
            from .utils import _gpu_present

            mode = "device" if _gpu_present() else "host"
        return mode

    def _evaluate(self, spectrum: bool, angles: np.ndarray, evaluate=None, workspace_bytes=None) -> np.ndarray:
        """Walk the DAG for every row of ``angles`` ``[B, n_params]``: -> complex128 ``[B, n_roots, F]`` on the host.
        The batch is cut into chunks whose node values fit ``workspace_bytes``; on the device every chunk is ONE call
        of ``qmle_fourier_dag`` for all its samples and all roots."""
        global TREE_LAUNCHES
        from . import _native as N

        mode = self._resolve_evaluate(evaluate)
        dag = self._ensure_dag()
        levels = self._levels(spectrum)
        dims = dag.dims if spectrum else []
        F = int(np.prod(dims, dtype=np.int64)) if dims else 1
        B, R = angles.shape[0], len(dag.roots)
        budget = int(workspace_bytes or self.workspace_bytes or TREE_WORKSPACE_BYTES)
        if mode == "device":
            one = N.fourier_workspace_bytes(dag.n_nodes, len(levels), R, F, 1)
            per = N.fourier_workspace_bytes(dag.n_nodes, len(levels), R, F, 2) - one
        else:
            per = 16 * (dag.n_nodes + 2) * F
            one = per
        if one == 0 or one > budget:
            raise FourierTreeTooLarge(
                f"one sample of this tree needs {one} bytes of workspace ({dag.n_nodes} nodes x {F} grid points x 16), "
                f"the budget is {budget}: pass a larger workspace_bytes")
        chunk = B if per == 0 else int(min(B, 1 + (budget - one) // per))
        out = np.empty((B, R, F), dtype=np.complex128)
        workspace = None
        for lo in range(0, B, chunk):
            part = angles[lo:lo + chunk]
            if mode == "device":
                if workspace is None:
                    torch = N.require_gpu()
                    need = N.fourier_workspace_bytes(dag.n_nodes, len(levels), R, F, min(chunk, B))
                    workspace = torch.empty((need,), dtype=torch.uint8, device=N.current_device())
                TREE_LAUNCHES += 1
                out[lo:lo + chunk] = N.to_host(N.fourier_dag(dag.nodes, levels, dag.roots, dag.root_phase, dims, part,
                                                             workspace=workspace))
            else:
                out[lo:lo + chunk] = self._evaluate_host(levels, dims, part)
        return out

    def _evaluate_host(self, levels: np.ndarray, dims: List[int], angles: np.ndarray) -> np.ndarray:
        """float64 NumPy interpreter of the tables, level by level, every node of a level and every sample at once."""
        from . import _native as N

        dag = self._ensure_dag()
        B, M = angles.shape[0], dag.n_nodes
        shape = tuple(dims)
        F = int(np.prod(shape, dtype=np.int64)) if shape else 1
        V = np.zeros((M + 2, B, F), dtype=np.complex128)  # rows M, M + 1: the terminals ZERO and ONE
        centre = int(sum((n - 1) // 2 * int(np.prod(shape[a + 1:], dtype=np.int64)) for a, n in enumerate(shape)))
        V[M + 1, :, centre] = 1.0
        row = lambda codes: np.where(codes >= 0, codes, M + 2 + codes)  # noqa: E731  (-2 -> M, -1 -> M + 1)
        i_pow = np.array([1, 1j, -1, -1j])

        def shifted(f: np.ndarray, axis: int, w: int) -> np.ndarray:
            """(T f)(omega) = f(omega - w e_axis) on the grid, zero where the source is outside."""
            g = f.reshape(f.shape[:2] + shape)
            out = np.zeros_like(g)
            src = [slice(None)] * g.ndim
            dst = [slice(None)] * g.ndim
            n = shape[axis]
            if abs(w) < n:
                dst[2 + axis] = slice(max(w, 0), n + min(w, 0))
                src[2 + axis] = slice(max(-w, 0), n + min(-w, 0))
                out[tuple(dst)] = g[tuple(src)]
            return out.reshape(f.shape)

        for lv in levels:
            b, e = int(lv["node_begin"]), int(lv["node_end"])
            if e == b:
                continue
            nd = dag.nodes[b:e]
            a, s = V[row(nd["cos_child"])], V[row(nd["sin_child"])]
            if lv["kind"] == N.FOURIER_KINDS["ANGLE"]:
                t = angles[:, int(lv["column"])]
                V[b:e] = np.cos(t)[None, :, None] * a + (i_pow[(nd["power"] + 1) & 3][:, None, None]
                                                         * np.sin(t)[None, :, None]) * s
            else:
                axis, w = int(lv["axis"]), int(lv["shift"])
                V[b:e] = 0.5 * (shifted(a, axis, w) + shifted(a, axis, -w)) \
                    + i_pow[nd["power"] & 3][:, None, None] * (0.5 * (shifted(s, axis, w) - shifted(s, axis, -w)))
        out = V[row(dag.roots.astype(np.int64))] * i_pow[dag.root_phase & 3][:, None, None]
        return np.ascontiguousarray(np.swapaxes(out, 0, 1))

    # ---- public evaluation ------------------------------------------------------------------------
    def __call__(self, params=None, inputs=None, force_mean: bool = False, evaluate: Optional[str] = None,
                 workspace_bytes: Optional[int] = None, **kwargs):
        """Expectation value(s) of the model's observables through the tree (equal to the circuit's).  With
        ``params=None`` the model's parameters are used (the first set of a batch, with a warning); explicit
        ``params`` may hold a batch of sets and ``inputs`` a batch of points: the result then has the model's layout
        ``(B_I, B_P, n_obs)`` without its axes of length 1."""
        if kwargs.get("execution_type", "expval") != "expval":
            raise NotImplementedError('Currently, only "expval" execution type is supported when building FourierTree. '
                                      f"Got {kwargs.get('execution_type', 'expval')}.")
        if kwargs.get("noise_params", None) is not None:
            raise NotImplementedError("Currently, noise is not supported when building FourierTree.")
        if params is None:
            params = self._single_param_set(self.model.params)
        else:
            params = self.model._params_validation(params)
        angles, B_I, B_P = self._canonical_angles(params, 1.0 if inputs is None else inputs)
        values = np.real(self._evaluate(False, angles, evaluate, workspace_bytes)[:, :, 0])  # [B, n_roots]
        if force_mean:
            values = values.mean(axis=1)
        if angles.shape[0] == 1:
            return values[0]
        return values.reshape((B_I, B_P) + values.shape[1:]).squeeze() if B_I * B_P == angles.shape[0] else values

    def get_spectrum(self, force_mean: bool = False, params=None, evaluate: Optional[str] = None,
                     workspace_bytes: Optional[int] = None) -> Tuple[List[np.ndarray], List[np.ndarray]]:
        """``(coefficients, frequencies)``, one entry per observable (one in all with ``force_mean``: the mean over
        the union of the roots' frequencies).  Frequencies are 1-D for one feature, ``(n_freq, d)`` otherwise, and
        are the structural support of the tree.  ``params``: a batch of parameter sets; the coefficients are then
        ``(B, n_freq)`` per entry."""
        batched = params is not None and np.ndim(params) > 2
        angles, _, _ = self._canonical_angles(self._params if params is None else params,
                                              np.ones(self.model.n_input_feat))
        dag = self._ensure_dag()
        grid = self._evaluate(True, angles, evaluate, workspace_bytes)  # [B, n_roots, F]
        freqs = self._dag_frequencies()
        coeffs = []
        for r, mask in enumerate(dag.masks):
            flat = [i for i in range(mask.bit_length()) if (mask >> i) & 1]
            c = grid[:, r, flat] if flat else np.zeros((grid.shape[0], 1), dtype=np.complex128)
            coeffs.append(c if batched else c[0])
        return self._combine_roots(coeffs, freqs, force_mean)

    def _combine_roots(self, per_root_coeffs, per_root_freqs, force_mean: bool):
        if not force_mean:
            return [np.asarray(c) for c in per_root_coeffs], [np.asarray(f) for f in per_root_freqs]
        keys = sorted({(int(v),) if np.ndim(f) == 1 else tuple(int(x) for x in v)
                       for f in per_root_freqs for v in np.asarray(f)})
        at = {k: i for i, k in enumerate(keys)}
        lead = np.shape(per_root_coeffs[0])[:-1] if per_root_coeffs else ()
        total = np.zeros(lead + (len(keys),), dtype=np.complex128)
        for c, f in zip(per_root_coeffs, per_root_freqs):
            f = np.asarray(f)
            cols = [at[(int(v),) if f.ndim == 1 else tuple(int(x) for x in v)] for v in f]
            np.add.at(total, (Ellipsis, cols), np.asarray(c))
        freq_arr = np.array(keys, dtype=np.int64).reshape(len(keys), -1)
        return [total / max(len(per_root_coeffs), 1)], [freq_arr[:, 0] if freq_arr.shape[1] == 1 else freq_arr]

    # ---- the explicit tree (host, lazily) ---------------------------------------------------------
    @property
    def leaf_arrays(self):
        """Per root ``(S, C, terms)``: the sine / cosine factor counts ``(n_leaves, n_params)`` of every leaf with a
        non-zero constant, and the constants ``<0| O_leaf |0>``."""
        self._ensure_structure()
        return self._leaf_arrays

    @property
    def weights_per_root(self):
        """Per root the ``(n_freq, n_leaves)`` matrix W with ``coefficients = W @ (terms * variational factors)``."""
        self._ensure_structure()
        return self._weights_per_root

    @property
    def freqs_per_root(self):
        self._ensure_structure()
        return self._freqs_per_root

    def _ensure_structure(self) -> None:
        if not self._structure_built:
            self._build_leaf_arrays()
            self._build_spectrum_structure()
            self._structure_built = True

    def _early_stopping_possible(self, pauli_idx: int, observable: PauliWord) -> bool:
        """Light-cone cut: an X/Y of the word on a qubit where no rotation 0..pauli_idx has an X/Y stays for good, so
        no leaf below is diagonal."""
        if pauli_idx < 0:
            return not observable.is_diagonal
        return bool(np.any(observable.xy_mask & ~self.cumulative_xy[pauli_idx]))

    def _build_leaf_arrays(self) -> None:
        """Enumerate the leaves of the tree, one path at a time.  A path is two bit masks over the rotations (which
        contributed a sine, which a cosine) and the phase of its leaf word; ``max_leaves`` bounds the walk."""
        paulis, observables = self._packed_words()
        K = self.n_params
        cum, running = [], 0
        for xp, _, _ in paulis:
            running |= xp
            cum.append(running)
        self._leaf_arrays = []
        budget = [self.max_leaves]

        def collect(idx, x, z, phase, s_mask, c_mask, leaves):
            while idx >= 0:
                if x & ~cum[idx]:
                    return
                xp, zp, _ = paulis[idx]
                if (_popcount(x & zp) + _popcount(z & xp)) & 1:
                    break
                idx -= 1
            else:
                if x == 0:
                    if budget[0] <= 0:
                        raise FourierTreeTooLarge(
                            f"the sine-cosine tree has more than max_leaves = {self.max_leaves} leaves; use "
                            'get_exact_support(method="dp") / exact_spectrum(method="dp"), which need no leaves '
                            "(get_spectrum never does)")
                    budget[0] -= 1
                    leaves.append((s_mask, c_mask, 1j ** phase))
                return
            xp, zp, php = paulis[idx]
            collect(idx - 1, x, z, phase, s_mask, c_mask | (1 << idx), leaves)
            collect(idx - 1, x ^ xp, z ^ zp, (phase + php + 2 * _popcount(zp & x)) & 3, s_mask | (1 << idx), c_mask,
                    leaves)

        old_limit = sys.getrecursionlimit()
        sys.setrecursionlimit(max(old_limit, 4 * K + 1000))
        try:
            for xo, zo, pho in observables:
                leaves: list = []
                collect(K - 1, xo, zo, pho, 0, 0, leaves)
                bits = lambda masks: np.array([[(m >> k) & 1 for k in range(K)] for m in masks],  # noqa: E731
                                              dtype=np.int64).reshape(len(masks), K)
                self._leaf_arrays.append((bits([s for s, _, _ in leaves]), bits([c for _, c, _ in leaves]),
                                          np.array([t for _, _, t in leaves], dtype=np.complex128)))
        finally:
            sys.setrecursionlimit(old_limit)

    def _build_spectrum_structure(self) -> None:
        """Per root the frequency vectors and W.  An input column with a cosine gives ``(e^{iwx} + e^{-iwx}) / 2``,
        with a sine ``i sin = (e^{iwx} - e^{-iwx}) / 2``; a leaf's input factors are multiplied out one column at a
        time.  A frequency whose terms cancel inside a leaf keeps its (zero) entry: the list is the structural
        support.  All weights are dyadic rationals, exact in float64."""
        d = len(self.features)
        axis_of = {f: a for a, f in enumerate(self.features)}
        columns = [(k, axis_of[f], int(self.input_scaling[k])) for f in self.features for k in self.input_indices[f]]
        self._freqs_per_root, self._weights_per_root = [], []
        for S, C, _ in self._leaf_arrays:
            n_leaves = S.shape[0]
            table: dict = {}
            for leaf in range(n_leaves):
                poly = {(0,) * max(d, 1): 1.0}
                for k, axis, w in columns:
                    if not (S[leaf, k] or C[leaf, k]):
                        continue
                    minus = -0.5 if S[leaf, k] else 0.5
                    grown: dict = {}
                    for omega, weight in poly.items():
                        for delta, factor in ((w, 0.5), (-w, minus)):
                            key = omega[:axis] + (omega[axis] + delta,) + omega[axis + 1:]
                            grown[key] = grown.get(key, 0.0) + weight * factor
                    poly = grown
                for omega, weight in poly.items():
                    table.setdefault(omega, np.zeros(n_leaves, dtype=np.complex128))[leaf] += weight
            if table:
                omegas = sorted(table)
                W = np.stack([table[o] for o in omegas])
                freqs = np.array(omegas, dtype=np.int64)
            else:
                freqs = np.zeros((1, max(d, 1)), dtype=np.int64)
                W = np.zeros((1, n_leaves), dtype=np.complex128)
            self._freqs_per_root.append(freqs[:, 0] if freqs.shape[1] == 1 else freqs)
            self._weights_per_root.append(W)

    def _leaf_factors(self, S: np.ndarray, C: np.ndarray, columns: np.ndarray) -> np.ndarray:
        """Per leaf ``prod_k cos(theta_k)^C (i sin(theta_k))^S`` over ``columns``, at the tree's current angles."""
        theta = np.array([float(self.parameters[k]) for k in columns], dtype=np.float64)
        cos, isin = np.cos(theta)[None, :], 1j * np.sin(theta)[None, :]
        return np.prod(np.where(C[:, columns] > 0, cos, 1.0) * np.where(S[:, columns] > 0, isin, 1.0), axis=1)

    # ---- exact support ------------------------------------------------------------------------------
    def get_exact_support(self, method: str = "tree") -> List[np.ndarray]:
        """The frequencies whose coefficient is not identically zero in the variational parameters, per root.
        ``"tree"`` is exact: every leaf's variational factor is a square-free monomial in ``cos`` / ``i sin`` of
        distinct parameters, monomials with different signatures are linearly independent, so a coefficient vanishes
        identically iff the (exact, dyadic) weights of every signature group sum to zero.  It enumerates leaves
        (``max_leaves``).  ``"dp"`` walks the merged DAG with sets of achievable input (sine, cosine) counts instead:
        cheap for deep circuits, one feature with unit scaling only, and a superset where paths with one signature
        cancel each other."""
        if method == "dp":
            return self._support_dp()
        if method != "tree":
            raise ValueError(f"Unknown method '{method}'. Use 'tree' or 'dp'.")
        self._ensure_structure()
        var = self.var_positions
        out = []
        for (S, C, terms), W, freqs in zip(self._leaf_arrays, self._weights_per_root, self._freqs_per_root):
            freqs = np.asarray(freqs)
            if S.shape[0] == 0:
                out.append(freqs[:0])
                continue
            groups: dict = {}
            for leaf in range(S.shape[0]):
                sig = (S[leaf, var].tobytes(), C[leaf, var].tobytes())
                groups[sig] = groups.get(sig, 0) + W[:, leaf] * terms[leaf]
            alive = np.any(np.abs(np.stack(list(groups.values()))) > 1e-12, axis=0)
            out.append(freqs[alive])
        return out

    def _support_dp(self) -> List[np.ndarray]:
        if len(self.features) != 1:
            raise NotImplementedError("The 'dp' support method currently supports exactly one input feature; use "
                                      "method='tree' for multi-feature models.")
        if self.all_input_indices and np.any(np.abs(self.input_scaling[self.all_input_indices]) != 1):
            raise NotImplementedError(
                "The 'dp' support method does not support non-unit input frequency scaling (it aggregates sin/cos "
                "counts and cannot represent per-gate scalings); use method='tree'.")
        dag = self._ensure_dag()
        stride = len(self.all_input_indices) + 1  # bit s * stride + c <-> s sines and c cosines of the input
        nodes = dag.nodes
        value = [0] * (dag.n_nodes + 2)  # slots -2, -1: the terminals ZERO (nothing) and ONE (no factor: bit 0)
        value[-1] = 1
        for k in range(self.n_params):
            is_input = k in dag.column_axis
            for j in range(int(dag.bounds[k]), int(dag.bounds[k + 1])):
                c, s = value[int(nodes["cos_child"][j])], value[int(nodes["sin_child"][j])]
                value[j] = ((c << 1) | (s << stride)) if is_input else (c | s)
        out = []
        for root in dag.roots:
            pairs, freqs = value[int(root)], set()
            while pairs:
                bit = (pairs & -pairs).bit_length() - 1
                freqs |= self._expansion_support(bit // stride, bit % stride)
                pairs &= pairs - 1
            out.append(np.array(sorted(freqs), dtype=np.int64))
        return out

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _expansion_support(s: int, c: int) -> frozenset:
        """Frequencies with a non-zero coefficient in ``cos^c(x) (i sin(x))^s``: those of ``(t - 1)^s (t + 1)^c``,
        ``t = e^{2ix}``, multiplied out in integers (``cos x sin x`` has no constant term)."""
        poly = [1]
        for sign, count in ((-1, s), (1, c)):
            for _ in range(count):
                poly = [(poly[i - 1] if i else 0) + sign * (poly[i] if i < len(poly) else 0)
                        for i in range(len(poly) + 1)]
        return frozenset(2 * k - (s + c) for k, a in enumerate(poly) if a != 0)


class _PairStats:
    """Pairwise-complete moments of the columns of ``mat`` (N observations x K variables):
    for every column pair (i, j) only rows finite in BOTH columns count -- the pandas
    ``corr`` convention the reference follows.  All sums are K x K matrix products."""

    def __init__(self, mat: np.ndarray) -> None:
        mat = np.asarray(mat)
        ok = np.isfinite(mat)
        x = np.where(ok, mat, 0)
        w = ok.astype(np.float64)
        self.nobs = w.T @ w
        n = np.where(self.nobs > 0, self.nobs, 1.0)
        sx = x.T @ w            # sum of column i over the rows valid for (i, j)
        sy = w.T @ x            # sum of column j over the same rows
        a2 = np.abs(x) ** 2
        self.sxy = np.conj(x).T @ x - np.conj(sx) * sy / n      # centred cross moment
        self.ssx = a2.T @ w - np.abs(sx) ** 2 / n
        self.ssy = w.T @ a2 - np.abs(sy) ** 2 / n

    def masked(self, result: np.ndarray, minp: int) -> np.ndarray:
        return np.where(self.nobs < minp, np.nan, result)


def _stack_complex(mat: np.ndarray) -> np.ndarray:
    """Complex samples count as two real samples (real parts, then imaginary parts)."""
    mat = np.asarray(mat)
    return np.concatenate([mat.real, mat.imag], axis=0) if np.iscomplexobj(mat) else mat


class FCC:
    """Fourier-coefficient correlation (arXiv:2508.20868); API of ``coefficients.py:966-1650``."""

    @classmethod
    def get_fcc(cls, model: Model, n_samples: int, random_key=None,
                method: Optional[str] = "pearson", scale: Optional[bool] = False,
                weight: Optional[bool] = False, trim_redundant: Optional[bool] = True,
                **kwargs) -> float:
        """Mean absolute correlation between the coefficients of different frequencies over
        ``n_samples`` random parameter sets (``coefficients.py:968-1044``)."""
        if trim_redundant and not weight:
            # positive-frequency block only; mean |r| over its strict lower triangle
            _, coeffs, freqs = cls._calculate_coefficients(model, n_samples, random_key, scale,
                                                           **kwargs)
            keep = cls._calculate_mask(freqs)
            block = np.abs(cls._correlate(coeffs.reshape(-1, coeffs.shape[-1])[keep].T,
                                          method=method))
            low = np.tril(np.ones(block.shape, dtype=bool), k=-1) & np.isfinite(block)
            # (the matrix is symmetric in magnitude: lower triangle == half the off-diagonal)
            return float(block[low].sum() / low.sum()) if low.any() else float("nan")
        fingerprint, _ = cls.get_fourier_fingerprint(
            model, n_samples, random_key, method, scale, weight, trim_redundant=trim_redundant,
            **kwargs)
        return cls.calculate_fcc(fingerprint)

    @classmethod
    def get_fourier_fingerprint(cls, model: Model, n_samples: int, random_key=None,
                                method: Optional[str] = "pearson", scale: Optional[bool] = False,
                                weight: Optional[bool] = False,
                                trim_redundant: Optional[bool] = True,
                                nan_to_one: Optional[bool] = False, **kwargs: Any):
        """Correlation matrix of the Fourier coefficients and its frequency labels
        (``coefficients.py:1047-1162``).  With ``trim_redundant`` only the strict lower
        triangle of the non-negative-frequency block survives and the labels are a
        ``(row_freqs, col_freqs)`` tuple."""
        _, coeffs, freqs = cls._calculate_coefficients(model, n_samples, random_key, scale,
                                                       **kwargs)
        keep = cls._calculate_mask(freqs) if trim_redundant else None
        if trim_redundant and not weight:
            fp = cls._correlate(coeffs.reshape(-1, coeffs.shape[-1])[keep].T, method=method)
        else:
            fp = cls._correlate(coeffs.transpose(), method=method)
        if nan_to_one:
            fp = np.where(np.isnan(fp), 1.0, fp)
        if weight:
            fp = cls._weighting_mean(fp, coeffs)
            if trim_redundant:
                fp = fp[keep][:, keep]
        if not trim_redundant:
            return fp, freqs
        labels = cls._flat_frequencies(freqs)[keep]
        fp = np.where(np.tril(np.ones(fp.shape, dtype=bool), k=-1), fp, np.nan)
        rows = np.any(np.isfinite(fp), axis=1)
        cols = np.any(np.isfinite(fp), axis=0)
        return fp[rows][:, cols], (labels[rows], labels[cols])

    @classmethod
    def calculate_fcc(cls, fourier_fingerprint: np.ndarray) -> float:
        """``nanmean(|fingerprint|)`` (``coefficients.py:1165-1180``)."""
        return float(np.nanmean(np.abs(fourier_fingerprint)))

    @classmethod
    def _calculate_mask(cls, freqs) -> np.ndarray:
        """Flat (C-order) indices of the coefficients whose frequency is non-negative on
        every input axis (``coefficients.py:1183-1229``)."""
        fa = np.asarray(freqs)
        if fa.ndim == 1:
            return np.flatnonzero(fa >= 0)
        nonneg = np.ones((), dtype=bool)
        for axis in fa:                       # outer "and" over the axes, C order
            nonneg = np.logical_and(nonneg[..., None], axis >= 0)
        return np.flatnonzero(nonneg.reshape(-1))

    @classmethod
    def _flat_frequencies(cls, freqs) -> np.ndarray:
        """Per-coefficient frequency labels in the same C order: the vector itself for one
        feature, ``(N, n_feat)`` tuples otherwise (``coefficients.py:1232-1254``)."""
        fa = np.asarray(freqs)
        if fa.ndim == 1:
            return fa
        return np.stack(np.meshgrid(*fa, indexing="ij"), axis=-1).reshape(-1, fa.shape[0])

    @classmethod
    def _calculate_coefficients(cls, model: Model, n_samples: int, random_key=None,
                                scale: bool = False, **kwargs: Any):
        """Re-draw ``n_samples`` (``x 2^n x n_features`` when ``scale``) parameter sets and
        return ``(params, coeffs, freqs)`` with the sample axis last
        (``coefficients.py:1257-1298``)."""
        if n_samples > 0:
            total = int(2**model.n_qubits * n_samples * model.n_input_feat) if scale else n_samples
            if scale:
                log.info("Using %d samples.", total)
            model.initialize_params(random_key, repeat=total)
        coeffs, freqs = Coefficients.get_spectrum(model, shift=True, trim=True, **kwargs)
        return model.params, coeffs, freqs

    @classmethod
    def _correlate(cls, mat: np.ndarray, method: str = "pearson") -> np.ndarray:
        """Correlate the columns of ``mat`` (samples x coefficients; extra coefficient axes
        are flattened in C order) -- ``coefficients.py:1301-1343``."""
        mat = np.asarray(mat)
        assert mat.ndim >= 2, "Input matrix must have at least 2 dimensions"
        fn = {"pearson": cls._pearson, "complex_pearson": cls._complex_pearson,
              "spearman": cls._spearman, "covariance": cls._covariance}.get(method)
        if fn is None:
            raise ValueError(
                f"Unknown correlation method: {method}. Must be 'pearson', "
                "'complex_pearson', 'spearman' or 'covariance'.")
        return fn(mat.reshape(mat.shape[0], -1))

    @classmethod
    def _covariance(cls, mat: np.ndarray, minp: Optional[int] = 1) -> np.ndarray:
        """Hermitian sample covariance ``sum conj(x_i - m_i)(x_j - m_j) / (nobs - 1)`` over
        pairwise-complete rows (``coefficients.py:1346-1395``)."""
        st = _PairStats(mat)
        return st.masked(st.sxy / np.where(st.nobs > 1, st.nobs - 1, np.nan), minp)

    @classmethod
    def _complex_pearson(cls, mat: np.ndarray, minp: Optional[int] = 1) -> np.ndarray:
        """Hermitian normalised covariance: ``|r_ij|`` = strength, ``angle(r_ij)`` = relative
        phase of column j against column i (``coefficients.py:1398-1453``)."""
        st = _PairStats(mat)
        denom = np.sqrt(st.ssx * st.ssy)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(denom > 0, st.sxy / np.where(denom > 0, denom, 1.0), np.nan)
            mag = np.abs(r)
            r = np.where(mag > 1.0, r / mag, r)
        return st.masked(r, minp)

    @classmethod
    def _pearson(cls, mat: np.ndarray, minp: Optional[int] = 1) -> np.ndarray:
        """``cov_ij / sqrt(cov_ii cov_jj)``, clipped to [-1, 1]; complex input is stacked
        as real + imaginary samples (``coefficients.py:1456-1497``)."""
        cov = cls._covariance(_stack_complex(mat), minp=minp)
        sd = np.sqrt(np.real(np.diagonal(cov)))
        denom = sd[:, None] * sd[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(denom > 0, np.real(cov) / np.where(denom > 0, denom, 1.0), np.nan)
        return np.clip(r, -1.0, 1.0)

    @classmethod
    def _spearman(cls, mat: np.ndarray, minp: Optional[int] = 1) -> np.ndarray:
        """Pearson correlation of the column-wise average ranks (non-finite entries are
        left out of the ranking) -- ``coefficients.py:1500-1579``."""
        mat = _stack_complex(mat)
        N, K = mat.shape
        if N < minp:
            return np.full((K, K), np.nan)
        ranks = np.full((N, K), np.nan)
        for j in range(K):
            ok = np.isfinite(mat[:, j])
            if ok.any():
                ranks[ok, j] = rankdata(mat[ok, j], method="average")
        st = _PairStats(ranks)
        denom = np.sqrt(st.ssx * st.ssy)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(denom > 0, np.real(st.sxy) / np.where(denom > 0, denom, 1.0), np.nan)
        return st.masked(np.clip(r, -1.0, 1.0), minp)

    @classmethod
    def _weighting_linear(cls, fourier_fingerprint: np.ndarray) -> np.ndarray:
        """Tent weights ``u_i + u_j``, ``u_k = (c - |k - c|) / (2c)``, c = centre (zero
        frequency) of an odd-sized fingerprint (``coefficients.py:1582-1614``)."""
        fp = np.asarray(fourier_fingerprint)
        assert fp.shape[0] % 2 != 0 and fp.shape[1] % 2 != 0, (
            "Correlation matrix must have odd dimensions. "
            "Hint: use `trim` argument when calling `get_spectrum`.")
        assert fp.shape[0] == fp.shape[1], "Correlation matrix must be square."
        c = fp.shape[0] // 2
        u = (c - np.abs(np.arange(fp.shape[0]) - c)) / (2 * c)
        return fp * (u[:, None] + u[None, :])

    @classmethod
    def _weighting_mean(cls, fourier_fingerprint: np.ndarray, coeffs: np.ndarray) -> np.ndarray:
        """Weights ``|mean_i| |mean_j|`` of the coefficient means over the samples, in the
        coefficient order ``_correlate`` uses (``coefficients.py:1617-1649``)."""
        fp, coeffs = np.asarray(fourier_fingerprint), np.asarray(coeffs)
        assert fp.shape[0] == fp.shape[1], "Correlation matrix must be square."
        assert coeffs.ndim >= 2, (
            "Coefficient matrix must contain coefficient axes and a sample axis.")
        m = np.abs(np.mean(coeffs, axis=-1)).T.reshape(-1)
        assert fp.shape[0] == m.shape[0], (
            "Correlation matrix size must match the number of Fourier coefficients.")
        return fp * m[:, None] * m[None, :]


class Datasets:
    """Synthetic training targets: a random real Fourier series on the model's own spectrum."""

    @classmethod
    def generate_fourier_series(cls, random_key, model: Model, coefficients_min: float = 0.0,
                                coefficients_max: float = 1.0, zero_centered: bool = False):
        """``[x, f(x), c]``: grid points ``(*degree, D)``, series values ``(*degree)`` and the
        (conjugate-symmetric, fftshift-ordered) coefficients ``(*degree)`` with
        ``fftshift(fftn(f)) == c`` (``coefficients.py:1654-1757``).  The flattened spectrum
        is ``[conj(c_M..c_1), c_0, c_1..c_M]`` with ``c_0`` real (or 0), drawn by
        :meth:`uniform_circle`."""
        D = model.n_input_feat
        grid = np.stack(np.meshgrid(*[np.arange(0, 2 * np.pi, 2 * np.pi / d)
                                      for d in model.degree])).T.reshape(-1, D)
        freqs = np.stack(np.meshgrid(*[np.asarray(f) for f in model.frequencies])).T.reshape(-1, D)
        half = cls.uniform_circle(random_key, size=math.prod(model.degree) // 2 + 1,
                                  low=coefficients_min, high=coefficients_max)
        half[0] = 0.0 if zero_centered else half[0].real
        coeffs = np.concatenate([np.conj(half[1:][::-1]), half])
        values = np.real((np.exp(1j * (grid @ freqs.T)) * coeffs).sum(axis=1) / coeffs.size)
        shape = tuple(model.degree)
        return [grid.reshape(*shape, -1), values.reshape(shape), coeffs.reshape(shape)]

    @classmethod
    def uniform_circle(cls, random_key, size, low: float = 0.0, high: float = 1.0) -> np.ndarray:
        """Complex numbers uniform on the disc / annulus: sqrt(U[low, high]) e^{2 pi i U}
        (``coefficients.py:1759-1788``)."""
        from .utils import as_key

        size = (size,) if isinstance(size, (int, np.integer)) else tuple(np.asarray(size).tolist())
        k_r, k_phi = as_key(random_key).split()
        r = np.sqrt(k_r.generator().uniform(low, high, size=size))
        return r * np.exp(2j * np.pi * k_phi.generator().uniform(size=size))

