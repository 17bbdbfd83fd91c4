/*
 * qmle_sv.h -- C ABI of libqmle_sv.so, the MI355X (gfx950) statevector engine
 * that replaces the compute seam of cirKITers/qml-essentials' "jaqsi" simulator.
 *
 * The reference is 100 % Python/JAX and has no FFI of its own (SURVEY.md F2,
 * 8-b).  The seam this ABI replaces is
 *
 *   simulation.simulate_and_measure(tape, n_qubits, type, obs, use_density)
 *        qml_essentials/simulation.py:131-139     (per-sample kernel)
 *   Script._execute_batched(type, obs, args, kwargs, in_axes)
 *        qml_essentials/script.py:399-408          (jax.vmap over the batch;
 *        script.py:443-453 marks it as the multi-device replacement point)
 *
 * Conventions (identical to the reference):
 *   - state = 2^n complex64 (float2, re/im interleaved), wire 0 = MOST significant
 *     bit of the flat index            (simulation.py:100-104, test_jaqsi.py:416-427)
 *   - a k-qubit gate on wires [w0..w(k-1)] has matrix row/col index
 *     sum_j bit[w_j] << (k-1-j)        (operations.py:38-50)
 *   - every execution starts from |0...0>   (simulation.py:100)
 *   - batch element b uses row b of the angle table (jax.vmap semantics,
 *     script.py:302-315); results carry a leading batch dimension.
 *
 * Ownership: the caller (PyTorch-ROCm in this repo) owns every device buffer;
 * the library owns only the plan.  No exceptions cross the ABI: 0 = ok, negative
 * = qmle_status.  Plans are immutable after creation except for a lazily created
 * device copy of their descriptors; one stream per call; no other global state.
 * All pointers named d_* are device pointers, everything else is host memory.
 * Batch limits: qmle_run_batch / _parity / _f64 take any batch >= 1 (they cut it into launches
 * themselves); the stand-alone kernels on resident states (qmle_expval_z, qmle_probs,
 * qmle_marginal_probs, qmle_meyer_wallach, qmle_overlap, qmle_expval_parity, qmle_density*,
 * qmle_apply_inplace*, qmle_sample_counts, qmle_probs_diag_expval) take batch <= 65535 per call
 * (one grid row per sample), qmle_adjoint_gradient batch <= 32767 -- QMLE_ERR_INVALID_ARG above
 * that; the Python host side slices longer batches (qml-essentials_amd/_native.py).
 */
#ifndef QMLE_SV_H
#define QMLE_SV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMLE_SV_VERSION 150 /* 0.1.4.9: plan flag 16 reserved (the prefetching tile kernel is gone), qmle_plan_create rejects it; (no version step: qmle_gram, qmle_gram_f64 and their workspace queries added); 0.1.4.8: qmle_adjoint_gradient_f64, k_direct_1q controlled-phase mode; 0.1.4.7: qmle_plan_executed (qmle_plan_expval_child = the folded child only); 0.1.4.6: qmle_plan_autotune; 0.1.4.5: QMLE_MEAS_MEYER_WALLACH; 0.1.4.4: qmle_philox_uniform_f32_device_key; 0.1.4.3: qmle_philox_uniform_f32_device; 0.1.4.2: qmle_apply_inplace_f64; 0.1.4.1: qmle_philox_uniform_f32 (host-side parameter sampler); 0.1.4: complex128 engine (qmle_run_batch_f64), qmle_meyer_wallach_reads, QMLE_ERR_INTERNAL; 0.1.3: fast tile path (no ABI change; a plan is bound to the device of its first run); 0.1.2: shot sampler; 0.1.1: qmle_op carries 4 wires (MAT4) */
#define QMLE_MAX_QUBITS 32

typedef struct qmle_plan qmle_plan;
typedef void *qmle_stream; /* hipStream_t */

typedef enum qmle_status {
  QMLE_OK = 0,
  QMLE_ERR_INVALID_ARG = -1,
  QMLE_ERR_WIRE_COUNT = -2,      /* operations.py:140-144  "expects k wire(s)" */
  QMLE_ERR_DUPLICATE_WIRES = -3, /* operations.py:145-146  "duplicate wires"   */
  QMLE_ERR_WIRE_RANGE = -4,      /* wire >= n_qubits                           */
  QMLE_ERR_UNKNOWN_OP = -5,
  QMLE_ERR_MEAS_TYPE = -6,       /* simulation.py:271 "Unknown measurement type" */
  QMLE_ERR_WORKSPACE = -7,       /* workspace too small                        */
  QMLE_ERR_HIP = -8,             /* a HIP runtime call failed                  */
  QMLE_ERR_NO_DEVICE = -9,
  QMLE_ERR_UNSUPPORTED = -10,
  QMLE_ERR_SLOT_RANGE = -11,
  QMLE_ERR_INTERNAL = -12        /* a build-time invariant of the kernels does not hold (e.g. a tile
                                    kernel whose dynamic LDS does not start at offset 0)          */
} qmle_status;

/* Gate vocabulary = the gate classes of qml_essentials/operations.py that the
 * 23 ansaetze, the encodings and the entanglement circuits put on the tape. */
typedef enum qmle_opcode {
  QMLE_OP_ID = 0,      /* operations.py:719  */
  QMLE_OP_X = 1,       /* PauliX  :746       */
  QMLE_OP_Y = 2,       /* PauliY  :762       */
  QMLE_OP_Z = 3,       /* PauliZ  :778       */
  QMLE_OP_H = 4,       /* :794               */
  QMLE_OP_S = 5,       /* :810               */
  QMLE_OP_RX = 6,      /* :1043  slot[0]=theta */
  QMLE_OP_RY = 7,      /* :1044              */
  QMLE_OP_RZ = 8,      /* :1045              */
  QMLE_OP_ROT = 9,     /* :1204  slot = phi,theta,omega */
  QMLE_OP_CX = 10,     /* :1098  wires = [control,target] */
  QMLE_OP_CY = 11,     /* :1099              */
  QMLE_OP_CZ = 12,     /* :1100              */
  QMLE_OP_CRX = 13,    /* :1485              */
  QMLE_OP_CRY = 14,    /* :1486              */
  QMLE_OP_CRZ = 15,    /* :1487              */
  QMLE_OP_CPHASE = 16, /* ControlledPhaseShift :1171 */
  QMLE_OP_SWAP = 17,   /* :831               */
  QMLE_OP_RXX = 18,    /* :1348              */
  QMLE_OP_RYY = 19,    /* :1349              */
  QMLE_OP_RZZ = 20,    /* :1350              */
  QMLE_OP_RZX = 21,    /* :1351              */
  QMLE_OP_CCX = 22,    /* :1103  wires = [c0,c1,target] */
  QMLE_OP_CSWAP = 23,  /* :1140  wires = [c,t0,t1]      */
  QMLE_OP_MAT1 = 24,   /* Operation(matrix=2x2), batch-constant; mat_off -> 8 floats  */
  QMLE_OP_MAT2 = 25,   /* Operation(matrix=4x4), batch-constant; mat_off -> 32 floats */
  QMLE_OP_DIAG_ALL = 26, /* DiagonalQubitUnitary on wires 0..n-1 in order (:922-926):
                            amp[i] *= exp(-i * consts[mat_off+i] * angle[slot0])
                            (Golomb encoding, unitary.py:661-701)              */
  QMLE_OP_MAT4 = 27,   /* dense 16x16 on 4 wires, batch-constant; mat_off -> 512 floats.
                          Superoperator of a 2-qubit Kraus channel on vec(rho)
                          (KrausChannel.apply_to_density, operations.py:1551-1578)   */
  QMLE_OP_MAT1_ROW = 28, /* Operation(matrix=[B,2,2]): one 2x2 per sample.  Its 8 numbers (row-major, re then im)
                            are the angle-table columns slot[0] .. slot[0] + 7; no reduction mod 4 pi */
  QMLE_OP_MAT2_ROW = 29, /* Operation(matrix=[B,4,4]): the same with 32 columns from slot[0] on */
  QMLE_OP__COUNT = 30
} qmle_opcode;

/* One tape entry.  Barriers (operations.py:964) are not sent: simulate_pure skips
 * them (simulation.py:93-94). */
typedef struct qmle_op {
  uint16_t opcode;  /* qmle_opcode */
  int16_t wire[4];  /* reference wire order; unused = -1 */
  int32_t slot[3];  /* column of the angle table per parameter; unused = -1 (MAT1_ROW / MAT2_ROW: slot[0] = first
                       of 8 / 32 consecutive columns) */
  int32_t mat_off;  /* float offset into `consts` for MAT1/MAT2/DIAG_ALL, else -1 */
} qmle_op;

/* measure_state types (simulation.py:204-271) + engine-internal extras */
typedef enum qmle_meas {
  QMLE_MEAS_STATE = 0,    /* out: [B][2^n] complex64                           */
  QMLE_MEAS_PROBS = 1,    /* out: [B][2^n] float32  |psi|^2                    */
  QMLE_MEAS_EXPVAL_Z = 2, /* out: [B][n_obs] float32, PauliZ on obs_wires[k]
                             (fast path simulation.py:241-261, all in ONE pass) */
  QMLE_MEAS_DENSITY = 3,  /* out: [B][2^n][2^n] complex64 = |psi><psi|
                             (simulation.py:183-189)                           */
  QMLE_MEAS_MEYER_WALLACH = 4 /* out: [B][n + 1] float32 = (Q, Tr rho_w^2 of wire 0 .. n-1):
                             Meyer-Wallach of the state the plan produces
                             (entanglement.py:56-103 + jaqsi.py:60-103).  The plan's last tile
                             pass reports the sums of its own tile from LDS -- for n <= 14 that
                             is everything and no state is stored; above, the state is stored
                             and the remaining positions cost ceil((n - T) / 8) further reads
                             (2 at n = 28) instead of qmle_meyer_wallach's 3.  batch chunks of
                             <= 65535 states are handled inside. */
} qmle_meas;

/* plan flags */
#define QMLE_PLAN_DEFAULT 0u
#define QMLE_PLAN_NO_FUSION 1u      /* one HBM pass per reference gate (roofline mode) */
#define QMLE_PLAN_FORCE_GLOBAL 2u   /* never use the whole-state-in-LDS kernel        */
#define QMLE_PLAN_FORCE_TILE 4u     /* never use the direct per-gate kernels          */
#define QMLE_PLAN_NO_REGTILE 8u     /* one LDS sweep per gate inside a tile (debug/A-B) */
                                    /* 16u: reserved -- qmle_plan_create returns QMLE_ERR_INVALID_ARG */
#define QMLE_PLAN_NO_MERGE 64u      /* keep every 1-qubit gate its own operator (no RY.RZ.RY products):
                                       the fused adjoint sweep needs one generator per gate */
#define QMLE_PLAN_NO_ABSORB 32u     /* <Z>: simulate trailing CX / SWAP / diagonal gates instead of
                                       folding them into the observables (A-B, tests)   */
#define QMLE_PLAN_NO_SPARSE 128u    /* runs from |0..0>: read and store every amplitude, launch every tile,
                                       even where the state is known to be exactly zero (A-B, tests) */
#define QMLE_PLAN_TAPE_ORDER (1u << 24) /* schedule commuting gates in tape order instead of low bit
                                          positions first (A-B, tests)                       */
/* bits 8..15: tile qubits T override (0 = auto); bits 16..23: low-bit count L override */
#define QMLE_PLAN_TILE_BITS(t) (((unsigned)(t) & 0xffu) << 8)
#define QMLE_PLAN_LOW_BITS(l) (((unsigned)(l) & 0xffu) << 16)

int qmle_sv_version(void);
const char *qmle_status_string(int status);
/* number of HIP devices visible (0 if none / no driver); never fails */
int qmle_device_count(void);

/* Validate + compile a tape into an execution plan (host only, no HIP calls).
 * consts: batch-constant floats referenced by mat_off (copied). */
int qmle_plan_create(const qmle_op *ops, int n_ops, int n_qubits, int n_slots,
                     const float *consts, int n_consts, unsigned flags,
                     qmle_plan **out);
int qmle_plan_destroy(qmle_plan *plan);
/* Opt-in plan autotuner (the default schedule is the pass-cost model's choice, deterministically).
 * Times the model's best `top_k` schedule candidates (x both paddings of the last stage) for THIS
 * measurement and batch size on the current device -- `reps` runs each, zero angles, its own scratch
 * (hipMalloc'ed and freed inside: a one-off step, not part of a hot loop) -- and re-schedules the plan
 * that qmle_run_batch executes to the fastest (it must win by 1 %).  Candidates are the same tape under
 * another tile geometry / order of commuting gates: results agree to float32 rounding.  meas_type:
 * QMLE_MEAS_STATE or QMLE_MEAS_EXPVAL_Z.  chosen[2] (optional) <- candidate index, padding; ms_before /
 * ms_after (optional) <- per-call times of the old and the new schedule.  Plans with a single schedule
 * (whole state in LDS, forced geometry, QMLE_PLAN_NO_FUSION) return QMLE_OK untouched (chosen = -1, -1).
 * If the scratch allocation fails the plan keeps its schedule, QMLE_OK is returned and chosen[1] = -2
 * ("not tuned": the caller may try again later).  A choice is remembered per (executed plan's tape,
 * flags, batch class, device) for the life of the process: where both measurement types execute the
 * same plan the first one tuned decides for both.  Callers that cached qmle_workspace_bytes must ask
 * again afterwards. */
int qmle_plan_autotune(qmle_plan *plan, int meas_type, int n_obs, int batch, int top_k, int reps,
                       qmle_stream stream, int32_t *chosen, double *ms_before, double *ms_after);

/* The plan QMLE_MEAS_EXPVAL_Z actually executes: trailing gates that permute basis states
 * linearly (CX, SWAP) or are diagonal are folded into the Z observables (Z_t -> Z_c Z_t),
 * the remaining gates form this child plan (owned by `plan`; NULL if nothing was folded).
 * For introspection / profiling only. */
qmle_plan *qmle_plan_expval_child(qmle_plan *plan);
/* The plan object qmle_run_batch really executes for `meas_type` (owned by `plan`, never NULL for a
 * valid plan): the folded child above for QMLE_MEAS_EXPVAL_Z, and of that / of the plan itself the
 * schedule compiled for runs from |0..0> when there is one (wider first tile; such a handle is refused
 * by qmle_apply_inplace and qmle_adjoint_gradient, which apply stages to LIVE states:
 * QMLE_ERR_UNSUPPORTED).  Describe, count stages of and profile THIS handle. */
qmle_plan *qmle_plan_executed(qmle_plan *plan, int meas_type);
/* JSON description of the compiled passes (for tests / DESIGN.md); returns the
 * number of bytes needed (excluding NUL); writes at most cap-1 bytes + NUL.
 * The description follows the handle's last run in two places: a schedule adopted by
 * qmle_plan_autotune, and stage 0's "write_bytes_from_zero".  A qmle_run_batch whose chunks share
 * workspace slots leaves out the zero fill of a chunk when the slot still holds the zeros of an
 * earlier chunk of the same call (all-live plans of two passes, <Z> measurements); stage 0 then reports the
 * bytes per state that run really wrote (its fills and first-tile stores over its states), and the
 * fresh-buffer figure 8 * 2^n before any run and after a run that filled every chunk or failed.  Describe the
 * handle of qmle_plan_executed, after the run.
 * The last stage also reports how the handle's last batch run went ("..._last_run"), among them
 * "chunk_loop_last_run": how that run ordered its chunks -- "one_stream" (one chunk, the whole state in the
 * LDS, QMLE_NO_CHUNK_OVERLAP=1, or no room for two slots), "staged" (two streams, stage k of a chunk behind
 * stage k of the chunk before it), "free" (two streams and no order between them: the runs that fill a slot once
 * per call, see qmle_workspace_bytes), "alone" (such runs of at least four chunks whose measuring launch streams
 * 1 GiB or more: one stream carries the measuring passes back to back and nothing else, the other every chunk's first
 * pass and epilogue; see qmle_chunk_loop_form), "none" before the first run.
 * Every tile stage lists "fast_ops", the ops of its fast-kernel stream (the concatenated "fast_groups") as
 * [dispatch code, float offset of the op's record in the per-sample matrix row], "unit_form_ops", the indices into
 * that stream of the ops applied in unit-pivot form, and "scale_carriers", the ops that take the product of the
 * pivots in front of them (see qmle_unit_form_chain).  "mat_floats_old" is the part of the row ("mat_floats") that
 * holds one plain record per operator, as every other kernel reads it; the records of unit-form ops and carriers
 * follow it and end at "mat_floats".  Behind them sit the product-form records of the fast groups: per stage,
 * "product_form_groups"[g] says whether fast group g runs in product form and "product_form_records"[g] gives the
 * float offset of its record (-1: none; see qmle_group_product_form); "mat_row_floats" is the row's stride.  A tile stage reports "group_product_form_last_run": its last launch ran those groups in
 * product form (the fast tile kernel always does; the generic tile kernel applies the plain records).
 * "closing_free_groups"[g]: a run that ends the stage in |amplitude|^2 only may build group g's record without a
 * closing diagonal (see qmle_group_product_form_measured); "measured_form_last_run": the last batch run did so for
 * its last stage and ran those records (false on every other stage and after every other kind of run).
 * "walk_kernel_last_run" (last stage): the fused <Z> pass of the last batch run ran in the straight-line kernel of
 * measuring walks whose groups all run in product form (see "walk_kernel" of qmle_plan_tile_route).
 * "mw_finish_last_run" (last stage): the finish of the last batch run's Meyer-Wallach calls behind the producing
 * pass -- "whole-state", "columns" or "per-position", the "finish" of qmle_meyer_wallach_describe -- and "" when
 * that run made no such call (another measurement, or the stand-alone reads of the stored states). */
int qmle_plan_describe(const qmle_plan *plan, char *buf, size_t cap);
/* Host only (no GPU needed): how tile stage `stage` of `plan` would run for a request -- the launch policy of the
 * tile passes as JSON, written like qmle_plan_describe (returns the bytes needed, or an error < 0: no tile stage
 * there, batch or meas out of range).  `meas`: what the pass does with the finished tile -- 0 store, 1
 * probabilities, 2 whole-state <Z>, 3 per-tile <Z> sums of every position, 4 per-tile Z-parity sums, 5 store +
 * Meyer-Wallach rows, 6 Meyer-Wallach rows alone.  `request_flags`: what the caller of the pass knows, QMLE_ROUTE_*.
 * Keys: "status" (0, or the error the launch would return), "family" (the kernel) and its instantiation ("dense4",
 * "mw", "nt", "measure", "multi", "ws", "masks", "mono_q", "pair"), "grid", "threads", "lds_bytes", "compact",
 * "tile_free", "mw_lean", "slots_in_lds", "fill" / "fill_elided" (a zero fill precedes the launch / is left out
 * because the zeros are in place), "tiles_per_workgroup", "row_shift" (a partial row covers 2^row_shift tiles),
 * the walk ("walk_slab", "walk_sync_staged", "walk_sync_tile_end", "staging_dma", "lane_swap",
 * "lane_swap_crossed"), "from_registers", "wave_private", "product_form", "walk_kernel" (the DMA walk with the last
 * group through lane swaps runs in a kernel of its own, because every group of the stage runs in product form; family,
 * instantiation keys, launch shape and rows stay those of the fast tile kernel).  A batch run reports what it did in
 * the "..._last_run" keys of qmle_plan_describe. */
#define QMLE_ROUTE_INIT_ZERO      1u   /* the pass starts from |0..0> instead of reading the states */
#define QMLE_ROUTE_FROM_ZERO      2u   /* the run started from |0..0> (every qmle_run_batch) */
#define QMLE_ROUTE_FOLD_COLS      4u   /* the fold-column buffer is there (every qmle_run_batch of a plan that wants it) */
#define QMLE_ROUTE_MULTI_ROWS     8u   /* the caller takes partial rows that cover several tiles */
#define QMLE_ROUTE_ZEROS_IN_PLACE 16u  /* the states already hold zeros outside tile 0 (an earlier chunk's fill) */
#define QMLE_ROUTE_SEMI_SINGLE    32u  /* each observable meets the last tile in at most one position */
#define QMLE_ROUTE_NO_MULTI_ZIN   64u  /* as if QMLE_NO_MULTI_ZIN were set */
#define QMLE_ROUTE_NO_MW_LEAN     128u /* as if QMLE_MW_NO_LEAN were set */
#define QMLE_ROUTE_MW_PER_POSITION 256u /* as if QMLE_MW_FINISH_PER_POSITION were set (qmle_meyer_wallach_describe) */
int qmle_plan_tile_route(const qmle_plan *plan, int stage, int batch, int meas, int n_obs, unsigned request_flags,
                         char *buf, size_t cap);
/* Host only: the matrix builder's unit-pivot chain for `n` given 2x2 matrices u[i] = {m00, m01, m10, m11} as
 * (re, im) doubles.  The fast tile kernel applies an eligible gate as U / pivot, a matrix with a literal 1 (48
 * packed instructions instead of 64), and the product P of a chain's pivots is folded into the chain's last gate,
 * the carrier.  Members 0 .. n-2 are unit-form ops (diag[i] != 0: a diagonal one; diag may be NULL), member n-1 is
 * the carrier.  records[i] = the 8 numbers of member i's record: dense {x, y, z, (form, 0)} with form 1 =
 * [[1, x], [y, z]] (pivot m00, taken when |m00| >= |m01|) and form 2 = [[x, 1], [y, z]] (pivot m01); diagonal
 * {1, 0, 0, m11 / m00}.  pivots[i] = member i's pivot (re, im); carrier = P u[n-1], plain layout. */
int qmle_unit_form_chain(const double *u, const int *diag, int n, double *records, double *pivots, double *carrier);
/* Host only: the matrix builder's product form of one register-tile group.  The group's n (1..4) uncontrolled
 * one-qubit operators u[i] = {m00, m01, m10, m11} as (re, im) doubles, each a scalar times a unitary, sit on the
 * distinct in-thread bits bits[i] (0..3) of a work item's 16 amplitudes.  Each factors as
 * g diag(1, l) [[c, -s], [s, c]] diag(1, r) with c, s >= 0; record (80 doubles): [0, 32) the opening diagonal, 16
 * complex numbers, the product of the r over the set bits of the amplitude's index; [32 + 2 b, 34 + 2 b) the real step
 * of bit b -- form 1 (c >= s, direct): (-t, u) with t = s / c, u = t / (1 + t^2), applied as a0 -= t a1, a1 += u a0;
 * form 2 (c < s, mirrored): (t', 0) with t' = c / s, applied as [[t', -1], [1, t']] --; [40 + b] the form of bit b
 * (0: no operator there); [48, 80) the closing diagonal, which carries g, l and the scales the real steps leave out.
 * forms[i] (may be NULL) = the form of operator i. */
int qmle_group_product_form(const double *u, const int *bits, int n, double *record, int *forms);
/* Host only: the same record in measured mode, as a <Z> or Z-parity batch run builds it for the groups of its last
 * stage that "closing_free_groups" marks (only basis permutations and |amplitude|^2 follow the group's wires, and no
 * unit-pivot chain is split).  The opening diagonal is the same; the real step of bit b is (-tau, s), tau = s / (1 + c)
 * <= 1, applied as a0 -= tau a1, a1 += s a0, a0 -= tau a1 -- the rotation itself, exactly; every form is 3; the
 * closing diagonal holds exact ones and record[44] = 1 says that it is not applied.  The record applies
 * D (x)_i u[i] / |g_i| for a diagonal D of unit phases.  "measured_form_last_run" of a plan's last stage reports
 * whether the last batch run built and ran such records. */
int qmle_group_product_form_measured(const double *u, const int *bits, int n, double *record, int *forms);
/* counts: [0]=reference gates, [1]=HBM passes, [2]=whole-state-LDS(0/1),
 * [3]=tile qubits T, [4]=floats of per-sample matrices, [5]=direct passes */
int qmle_plan_stats(const qmle_plan *plan, int64_t stats[8]);

/* Minimum workspace for `batch` samples and the bytes that let the engine keep
 * `states_in_flight` states resident (0 = engine default).  A batch larger than one chunk of that many
 * states is run with TWO chunks in flight, one stage apart, on two streams the library owns (they fork from
 * `stream` by an event and join it again before the call returns its last launch: to the caller the call is
 * ordered on `stream` like any other); the figure returned includes the second set of state buffers.  A
 * smaller workspace is legal: the engine splits what it gets in two, or keeps one chunk on `stream` alone.
 * Runs that fill a workspace slot once per call (two tile passes, <Z> out of the second) let the two streams run
 * free instead: each takes its chunks back to back, and the end of one chunk's measuring pass is covered by the
 * other stream's.  QMLE_NO_CHUNK_OVERLAP=1 (read per call): always the one-stream loop.
 * Between calls the caller owns the workspace, so every call fills its slots again -- unless the caller hands the
 * zeros back: qmle_run_batch_w / qmle_run_batch_map_w take `ws_token`, a HOST pointer (in / out, may be NULL) to a
 * value that is opaque to the caller.  A call that returns QMLE_OK writes the token of the workspace as it leaves it;
 * every error return writes 0.  Passing a non-zero token asserts two things: nobody wrote the workspace since the
 * call that produced the token, and this call is ordered behind that call (same stream, or an event between them).
 * Then the slots start as that call left them and the fills they no longer need are left out (the runs above that
 * fill a slot once per call: none is left).  The token carries a fingerprint of the schedule (qmle_plan_autotune
 * changes it), n, batch, measurement, the chunk size and slots, and the size and address of the aligned workspace;
 * a token with another fingerprint counts as 0, and NULL or 0 gives the behaviour of the entries without it.  The
 * engine keeps no record of workspaces: the token is all there is, and it belongs to the buffer it was made for. */
size_t qmle_workspace_bytes(const qmle_plan *plan, int batch, int meas_type,
                            int n_obs, int states_in_flight);
/* Host only (no GPU needed): how a batch run would order its chunks -- the "chunk_loop_last_run" value of
 * qmle_plan_describe -- for a 256-byte-aligned workspace of exactly the size qmle_workspace_bytes answers for these
 * arguments, given that the library's two streams can be made.  QMLE_NO_CHUNK_OVERLAP is read as by a run.  Of the
 * runs that fill a workspace slot once per call, "alone" is taken by those with at least four chunks whose chunk
 * holds 1 GiB of states or more (in_flight * 8 * 2^n): their measuring pass runs at the memory's rate, and two of
 * them at once are slower than one after the other.  A static string; "none" for arguments no run would accept. */
const char *qmle_chunk_loop_form(const qmle_plan *plan, int batch, int meas_type, int states_in_flight);

/* simulate_and_measure over a batch: d_angles is [batch][n_slots] float32,
 * d_out as documented per qmle_meas.  obs_wires is HOST memory.  */
int qmle_run_batch(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                   const int32_t *obs_wires, int n_obs, void *d_out, void *d_workspace,
                   size_t workspace_bytes, qmle_stream stream);
/* qmle_run_batch with the workspace token of qmle_workspace_bytes (above); ws_token == NULL: qmle_run_batch. */
int qmle_run_batch_w(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                     const int32_t *obs_wires, int n_obs, void *d_out, void *d_workspace,
                     size_t workspace_bytes, qmle_stream stream, uint64_t *ws_token);
/* Same, for Z (x) Z (x) .. parity observables (jaqsi.py:149-167; Model with tuple
 * output_qubit, model.py:980-990): wire_masks[k] (HOST) has bit w set iff wire w takes part.
 * Measured like QMLE_MEAS_EXPVAL_Z -- out of the last pass, no stored state; d_out
 * float32 [batch][n_obs]; workspace as for QMLE_MEAS_EXPVAL_Z. */
int qmle_run_batch_parity(qmle_plan *plan, const float *d_angles, int batch,
                          const uint32_t *wire_masks, int n_obs, float *d_out, void *d_workspace,
                          size_t workspace_bytes, qmle_stream stream);
/* ... with the workspace token (qmle_workspace_bytes); ws_token == NULL: qmle_run_batch_parity.  Plain Z's and
 * parities of one plan, batch and workspace share their tokens: the measurement type is the same. */
int qmle_run_batch_parity_w(qmle_plan *plan, const float *d_angles, int batch,
                            const uint32_t *wire_masks, int n_obs, float *d_out, void *d_workspace,
                            size_t workspace_bytes, qmle_stream stream, uint64_t *ws_token);

/* Angle table from DEVICE-resident arguments: out[b][s] = const[s] + sum_t coef[t] *
 * leaf_{arg[t]}[row_k(b)][idx[t]], terms of slot s = [ptr[s], ptr[s+1]); row_k(b) =
 * ((b + batch_offset) / div_k) % mod_k  (cartesian inputs x params batch, model.py:1449-1481).
 * d_leaves / strides / div / mod are HOST arrays of n_leaves <= 8 entries; everything d_* is
 * device memory.  The sum runs in fp64; d_period (may be NULL) holds one double per slot: where
 * > 0, a sum beyond +-period is reduced into [-period/2, period/2] before the float32 store; a sum
 * within +-period, the bounds included, is stored as it is (4 pi for the rotation gates, which depend on angle / 2 only -- binary / ternary encodings scale inputs
 * by up to 3^(n-1), ansaetze/encodings of model.py:804-816).  Replaces the host-side angle
 * arithmetic when params / inputs already live in HBM.  batch_offset < 0: QMLE_ERR_INVALID_ARG
 * (qmle_run_batch_map / _w answer the same for map->batch_offset < 0), before any launch. */
int qmle_build_angles(const float *const *d_leaves, const int64_t *leaf_strides,
                      const int32_t *leaf_div, const int32_t *leaf_mod, int n_leaves,
                      const int32_t *d_ptr, const int32_t *d_arg, const int32_t *d_idx,
                      const float *d_coef, const float *d_const, const double *d_period,
                      int n_slots, int64_t batch, int64_t batch_offset, float *d_out,
                      qmle_stream stream);

/* qmle_build_angles + qmle_run_batch behind ONE call (the Model's device route: its angle map is all the
 * host holds, model.py:804-816 / ansaetze.py:323-371).  `map` carries qmle_build_angles' arguments;
 * d_angles [batch][plan n_slots] float32 is SCRATCH: the call may fill and read it (fewer than 64 samples, or
 * a plan with the Golomb diagonal, which reads its angle in the pass itself) or leave it untouched -- from 64
 * samples on the per-sample gate matrices are built straight from the map (same arithmetic, same results
 * bit for bit, one kernel and the table's round trip less).  May be NULL for a plan without slots.  The
 * host's time between the two launches -- 8-14 us of an idle GPU in the 0.2 ms analysis loops of BASELINE
 * configs 3 / 4 -- is gone either way. */
typedef struct qmle_angle_map {
  const float *const *d_leaves;   /* HOST array of n_leaves device pointers */
  const int64_t *leaf_strides;    /* HOST */
  const int32_t *leaf_div;        /* HOST */
  const int32_t *leaf_mod;        /* HOST */
  int32_t n_leaves;
  const int32_t *d_ptr, *d_arg, *d_idx;
  const float *d_coef, *d_const;
  const double *d_period;         /* may be NULL */
  int64_t batch_offset;
} qmle_angle_map;
int qmle_run_batch_map(qmle_plan *plan, const qmle_angle_map *map, float *d_angles, int batch,
                       int meas_type, const int32_t *obs_wires, int n_obs, void *d_out,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream);
/* ... with the workspace token (qmle_workspace_bytes); ws_token == NULL: qmle_run_batch_map. */
int qmle_run_batch_map_w(qmle_plan *plan, const qmle_angle_map *map, float *d_angles, int batch,
                         int meas_type, const int32_t *obs_wires, int n_obs, void *d_out,
                         void *d_workspace, size_t workspace_bytes, qmle_stream stream, uint64_t *ws_token);

/* Apply the plan's passes in place to resident states [batch][2^n] complex64 (no
 * initialisation, no measurement) -- the per-gate loop simulation.py:102-103 alone.
 * Workspace: qmle_workspace_bytes(plan, batch, QMLE_MEAS_STATE, 0, 0). */
int qmle_apply_inplace(qmle_plan *plan, const float *d_angles, int batch, void *d_states,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream);

/* ---- complex128 execution (the reference's jax_enable_x64 mode, operations.py:12-16; switched on
 * by tests/test_coefficients.py:19, test_entanglement.py:13, test_ansaetze.py:18) ----------------
 * Same plan, same tape: angles float64 [batch][n_slots]; out = [B][2^n] complex128 (STATE),
 * [B][2^n] float64 (PROBS), [B][n_obs] float64 (EXPVAL_Z; wire_masks[k] has bit w set iff wire w
 * takes part in the Z (x) Z ... observable k -- HOST array), [B][2^n][2^n] complex128 (DENSITY,
 * n <= 12).  Every gate of the tape is applied (no observable folding, no known-zero shortcuts):
 * the accuracy mode, 1e-10 against a complex128 reference.  n <= 13: the state stays in LDS for
 * the whole circuit; above, one streaming pass per (merged) operator. */
int qmle_run_batch_f64(qmle_plan *plan, const double *d_angles, int batch, int meas_type,
                       const uint32_t *wire_masks, int n_obs, void *d_out, void *d_workspace,
                       size_t workspace_bytes, qmle_stream stream);
size_t qmle_workspace_bytes_f64(const qmle_plan *plan, int batch, int meas_type);
/* optional: the batch-constant blob of qmle_plan_create at full precision (explicit matrices of a
 * complex128 caller); same length, before the first qmle_run_batch_f64 of the plan */
int qmle_plan_set_consts_f64(qmle_plan *plan, const double *consts, int n_consts);
/* complex128 counterpart of qmle_apply_inplace: the plan's operators on resident states
 * [batch][2^n] complex128 (batch <= 65535 per call), no initialisation, no measurement.  The
 * doubled-register density-matrix path uses it between Kraus channels in x64 mode
 * (simulation.py:107-128). */
int qmle_apply_inplace_f64(qmle_plan *plan, const double *d_angles, int batch, void *d_states,
                           void *d_workspace, size_t workspace_bytes, qmle_stream stream);
size_t qmle_apply_inplace_f64_workspace_bytes(const qmle_plan *plan, int batch);

/* ---- dense matrices on three and four wires (products of gates, a user's Operation(wires, matrix), evolved
 * unitaries of three- and four-wire Hamiltonians) -- no plan, one streaming pass ---------------------------------
 * Applies one dense 2^k x 2^k matrix, k = 3 or 4, in place to `batch` resident states [batch][2^n]: complex64
 * (f64 = 0, float32 arithmetic) or complex128 (f64 = 1).  One read and one write of the state.
 * wires: HOST array of k wires in operation order -- the first wire is the most significant bit of the matrix index
 * (operations.embed_matrix), wire w is bit position n - 1 - w.  d_mats: DEVICE, complex128 row-major, [1][d][d]
 * (per_sample = 0: one matrix for every state) or [batch][d][d] (per_sample = 1: state b takes matrix b); rounded to
 * float32 for complex64 states.  The matrix need not be unitary.  Any batch >= 1 (the library splits launches).
 * Status codes, all before any device work: QMLE_ERR_UNSUPPORTED for k outside {3, 4} (matrices on five or more
 * wires are not served; one and two wires go through a plan); QMLE_ERR_INVALID_ARG for NULL pointers, batch < 1,
 * n < k, n > QMLE_MAX_QUBITS, f64 or per_sample outside {0, 1}; QMLE_ERR_WIRE_RANGE for a wire outside 0..n-1;
 * QMLE_ERR_DUPLICATE_WIRES.  The pass is no part of a plan: the adjoint sweep, compiled calls and the
 * density-matrix path do not take it (gradients through such gates, noisy tapes and compiled calls stay refused by
 * the front end). */
int qmle_apply_matrix(void *d_states, int n_qubits, int batch, int f64, const int32_t *wires, int k,
                      const void *d_mats, int per_sample, qmle_stream stream);

/* ---- matrix cotangents of a dense gate on three or four wires (the adjoint sweep's share of such a gate) --------
 * For psi and lambda, the sweep's states BEHIND a gate U on `wires` (k = 3 or 4, wire order and matrix index as for
 * qmle_apply_matrix), writes d_cot[b][a][c] = G[a][c] with
 *     M[a][c] = sum_rest conj(lambda[a, rest]) psi[c, rest],   G = M (U^+)^T,
 * so that dC/dtheta = 2 Re sum_ac G[a][c] dU[a][c]/dtheta.  d_psi, d_lam: DEVICE, [batch][2^n], complex64 (f64 = 0) or
 * complex128 (f64 = 1); both are read once and never written.  d_cot: DEVICE, [batch][d][d] in the states' precision.
 * d_mats: DEVICE, complex128, the FORWARD matrix, [1][d][d] (per_sample = 0) or [batch][d][d] (per_sample = 1);
 * NULL: d_cot receives M itself.  The moment is a product on the matrix cores (v_mfma_f32_16x16x4_f32 /
 * v_mfma_f64_16x16x4_f64) with per-block partial sums in the workspace and one finishing kernel that adds them in
 * double in a fixed order: no atomics, the same bits from call to call.  Any batch >= 1 (the library splits
 * launches).  Status codes as qmle_apply_matrix, all before any device work, NULL d_psi / d_lam / d_cot / d_ws being
 * QMLE_ERR_INVALID_ARG; a workspace smaller than qmle_wide_moment_workspace_bytes (0 for arguments the call would
 * refuse) is QMLE_ERR_WORKSPACE. */
int qmle_wide_moment(const void *d_psi, const void *d_lam, int n_qubits, int batch, int f64, const int32_t *wires,
                     int k, const void *d_mats, int per_sample, void *d_cot, void *d_ws, size_t ws_bytes,
                     qmle_stream stream);
size_t qmle_wide_moment_workspace_bytes(int n_qubits, int batch, int k, int f64);

/* ---- Kraus maps on three and four wires of a resident vec(rho): wide gates and wide channels of a noisy tape -----
 * rho -> sum_m K_m rho K_m^+ on k = 3 or 4 SYSTEM wires, in place, one read and one write of vec(rho) per call.  With
 * one unitary K it is an explicit matrix gate on a noisy tape, with a Kraus set a channel.
 * d_rho: DEVICE, [batch][4^n], vec(rho)[i * 2^n + j] = rho[i, j] (a register of 2n wires, the ket wires first),
 * complex64 (f64 = 0, float32 arithmetic) or complex128 (f64 = 1).  n_qubits: the number of SYSTEM qubits,
 * k <= n and 2n <= QMLE_MAX_QUBITS.  wires: HOST array of k system wires in operation order, the first one the most
 * significant bit of the operator index (as for qmle_apply_matrix); the ket bit of wire w sits on position
 * 2n - 1 - w of the register, the bra bit on n - 1 - w.  d_ops: DEVICE, complex128 row-major, [n_ops][d][d], d = 2^k
 * (per_sample = 0), or [batch][d][d] with n_ops = 1 (per_sample = 1: sample b takes operator b); rounded to float32
 * for complex64.  The operators need not be unitary nor sum to a trace-preserving map.
 * form: 1 = sandwich: every d x d block R of rho on the target bits becomes sum_m K_m R K_m^+ by two products per
 * operator on the matrix cores (2 d n_ops complex multiply-adds per amplitude); 2 = superoperator: the library
 * builds S = sum_m K_m (x) conj(K_m) (d^2 x d^2, index order of KrausChannel.superoperator up to the permutation
 * that sorts the wires, summed in float64 in the order of m) into the workspace and applies vec(R') = S vec(R)
 * (d^2 multiply-adds per amplitude whatever n_ops is); 0 = automatic: the sandwich for per_sample = 1, for one
 * operator at k = 3 and for up to four at k = 4 -- where the measured times of the two cross (profiles/density_wide.md;
 * their arithmetic breaks even later, at n_ops = d / 2).  qmle_density_apply_wide_form returns what 0 selects
 * (host only), or the status the call would return for these three arguments.
 * No atomics, fixed summation orders: the same bits from call to call.  Any batch >= 1 (the library splits launches).
 * Status codes, all before any device work: QMLE_ERR_UNSUPPORTED for k outside {3, 4}; QMLE_ERR_INVALID_ARG for NULL
 * pointers, batch < 1, n < k, 2n > QMLE_MAX_QUBITS, f64 / per_sample / form out of range, n_ops < 1, per_sample = 1
 * with n_ops != 1 or with form = 2, form = 1 with more than d^2 operators; QMLE_ERR_WIRE_RANGE;
 * QMLE_ERR_DUPLICATE_WIRES; QMLE_ERR_WORKSPACE for a workspace smaller than the query's answer (0 for arguments
 * the call would refuse).  Not served: five or more wires, the adjoint sweep (qmle_adjoint_density knows no such
 * step), compiled calls. */
int qmle_density_apply_wide(void *d_rho, int n_qubits, int batch, int f64, const int32_t *wires, int k,
                            const void *d_ops, int n_ops, int per_sample, int form, void *d_ws, size_t ws_bytes,
                            qmle_stream stream);
size_t qmle_density_apply_wide_workspace_bytes(int n_qubits, int batch, int k, int n_ops, int f64, int form);
int qmle_density_apply_wide_form(int k, int n_ops, int per_sample);

/* Optional per-pass HIP-event timing (bench.py's live roofline measurement): between
 * begin and end every pass launch of this plan is bracketed by an event pair on the
 * launch stream.  end() synchronises, fills stage_ms[i] / stage_launches[i] (i = pass
 * index of qmle_plan_describe) and returns 1 if `capacity` pairs were not enough. */
int qmle_profile_begin(qmle_plan *plan, int capacity);
int qmle_profile_end(qmle_plan *plan, double *stage_ms, int64_t *stage_launches, int n_stages);

/* ---- stand-alone measurement / analysis kernels on resident states ---------- */
/* d_states: [batch][2^n] complex64 */
int qmle_expval_z(const void *d_states, int n_qubits, int batch, const int32_t *obs_wires,
                  int n_obs, float *d_out, void *d_workspace, size_t workspace_bytes,
                  qmle_stream stream);
size_t qmle_expval_workspace_bytes(int n_qubits, int batch);
int qmle_probs(const void *d_states, int n_qubits, int batch, float *d_out,
               qmle_stream stream);
int qmle_density(const void *d_states, int n_qubits, int batch, void *d_out,
                 qmle_stream stream);
/* probs marginalised onto `keep` wires, kept wires in ascending wire order
 * (jaqsi.py:106-146): d_out [batch][2^n_keep] float32 (zeroed by the call) */
int qmle_marginal_probs(const void *d_states, int n_qubits, int batch,
                        const int32_t *keep_wires, int n_keep, float *d_out,
                        qmle_stream stream);
/* F_i = |<psi_i|psi_{i+n_pairs}>|^2, i < n_pairs; d_states holds 2*n_pairs states
 * (Expressibility pairing rule, expressibility.py:49-52; pure-state form of
 * math.py:60-86) */
int qmle_pair_fidelity(const void *d_states, int n_qubits, int n_pairs, float *d_out,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream);
size_t qmle_pair_fidelity_workspace_bytes(int n_qubits, int n_pairs);
/* Measurements of a vectorised density matrix (2n-"qubit" register, ket wires first:
 * the layout of Operation.apply_to_density, operations.py:485-512): diagonal
 * probabilities [batch][2^n] (measure_density "probs", simulation.py:303-304) and <Z> on
 * obs_wires from that diagonal. */
int qmle_density_probs(const void *d_rho, int n_qubits, int batch, float *d_out,
                       qmle_stream stream);
int qmle_density_expval_z(const void *d_rho, int n_qubits, int batch, const int32_t *obs_wires,
                          int n_obs, float *d_out, qmle_stream stream);
/* <a_i|b_i> for i < count (complex64 out[count]); the matrix-free general
 * observable path: <O> = Re <psi | O psi>  (simulation.py:263-269) */
int qmle_overlap(const void *d_a, const void *d_b, int n_qubits, int count, void *d_out,
                 void *d_workspace, size_t workspace_bytes, qmle_stream stream);
size_t qmle_overlap_workspace_bytes(int n_qubits, int count);
/* Z (x) Z (x) ... parity observables (jaqsi.py:149-167): wire_masks[k] has bit w set
 * iff wire w takes part in observable k (HOST array); d_out [batch][n_obs] float32 */
int qmle_expval_parity(const void *d_states, int n_qubits, int batch, const uint32_t *wire_masks,
                       int n_obs, float *d_out, void *d_workspace, size_t workspace_bytes,
                       qmle_stream stream);
size_t qmle_expval_parity_workspace_bytes(int n_qubits, int batch);
/* Pauli-word observables in one pass over the state (X / Y / Hermitian observables, operations.py:421-460
 * and simulation.py:263-269, any wire count): every such observable is a real-weighted sum of words.
 *   d_out[b][o] = sum over terms t with obs == o of coef_t * <psi_b| P_t |psi_b>,
 *   P = i^popcount(x & z) * X^x * Z^z   (so Y = i X Z per wire);  a column without a term is 0.
 * `terms` is a HOST array of 1..65536 entries, n_obs 1..4096, n_qubits 1..30, any batch (cut into launches
 * inside).  d_out float32 (complex64 states) / float64 (complex128 states) [batch][n_obs].  Terms whose X/Y
 * factors together touch at most 8 bit positions above the lowest 4 share ONE read of the state (up to 12
 * qubits: always one); a word with more X/Y factors than that is streamed with its partner amplitudes (two
 * reads per distinct x mask, shared by every term with that mask).  Partial sums -- one fp64 slot per wave of
 * a 2^12-amplitude tile, n_obs * max(1, 2^(n_qubits - 12)) * 4 slots per state of a launch (at most 65535 states)
 * -- go to the workspace and are added in fixed order in fp64: the same bits from call to call.  The workspace
 * therefore grows with n_obs * 2^n_qubits / 128 bytes per state (6 MiB for 47 observables at 24 qubits, 512 MiB
 * for 4096): callers with many observables on large registers pass fewer states per call.  QMLE_ERR_INVALID_ARG, before any device work, for NULL pointers,
 * counts out of range, an `obs` outside [0, n_obs) and a workspace smaller than the query's answer;
 * QMLE_ERR_WIRE_RANGE for a mask bit at or above n_qubits. */
typedef struct qmle_pauli_term {
  uint32_t x_wires, z_wires; /* bit w = wire w; X: x only, Z: z only, Y: both */
  int32_t obs;               /* which output column this term adds to */
  double coef;               /* real weight */
} qmle_pauli_term;
int qmle_expval_pauli(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms,
                      int n_terms, int n_obs, float *d_out, void *d_ws, size_t ws_bytes, qmle_stream stream);
int qmle_expval_pauli_f64(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms,
                          int n_terms, int n_obs, double *d_out, void *d_ws, size_t ws_bytes,
                          qmle_stream stream);
size_t qmle_expval_pauli_workspace_bytes(int n_qubits, int batch, int n_terms, int n_obs);
size_t qmle_expval_pauli_workspace_bytes_f64(int n_qubits, int batch, int n_terms, int n_obs);
/* host only, like qmle_meyer_wallach_reads: how many times the call streams the state from HBM (or the
 * negative status the call itself would return for these terms) */
int qmle_expval_pauli_reads(int n_qubits, const qmle_pauli_term *terms, int n_terms, int f64);
/* Applying a weighted sum of words to resident states -- lambda = H psi, the seed of the adjoint sweep for any
 * observable list that qmle_expval_pauli measures:
 *   d_out[b] = (sum_t d_weights[b][terms[t].obs] * terms[t].coef * P_t) d_states[b],
 *   (P psi)[i] = i^ny * (-1)^popcount((i ^ x) & z) * psi[i ^ x],  ny = popcount(x & z)  (x, z as bit positions).
 * d_weights [batch][n_obs] float32 (float64 for _f64) on the DEVICE, d_out complex64 (complex128) [batch][2^n];
 * `terms` as above (HOST array, 1..65536 entries, n_obs 1..4096, n_qubits 1..30), any batch (cut into launches of at
 * most 65535 states inside).  Terms with equal (x, z) are merged into unique words; a small kernel adds the
 * per-sample coefficient of every word in fp64 (stored in the precision of the states); a word whose terms cancel
 * and a column without a term contribute zero.  The words go through the planner of qmle_expval_pauli: a list
 * that is measured in one pass is applied in one pass (one read of psi, one write of lambda), every further pass
 * and every streamed x mask reads psi once more and reads and rewrites lambda.  No atomics: the same bits from
 * call to call.  The word and coefficient tables live in the workspace (about terms * (48 + 4 or 8 * states of a launch)
 * bytes, see the query).  The argument checks and statuses of qmle_expval_pauli, before any device work; in
 * addition d_out == d_states is QMLE_ERR_INVALID_ARG (partners are read after neighbours are written). */
int qmle_apply_pauli_sum(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms, int n_terms,
                         int n_obs, const float *d_weights, void *d_out, void *d_ws, size_t ws_bytes,
                         qmle_stream stream);
int qmle_apply_pauli_sum_f64(const void *d_states, int n_qubits, int batch, const qmle_pauli_term *terms,
                             int n_terms, int n_obs, const double *d_weights, void *d_out, void *d_ws,
                             size_t ws_bytes, qmle_stream stream);
size_t qmle_apply_pauli_sum_workspace_bytes(int n_qubits, int batch, int n_terms, int n_obs);
size_t qmle_apply_pauli_sum_workspace_bytes_f64(int n_qubits, int batch, int n_terms, int n_obs);
/* host only: reads of the state per call -- passes + 2 per streamed x mask, counted on the merged words (or the
 * negative status the call itself would return for these terms) */
int qmle_apply_pauli_sum_reads(int n_qubits, const qmle_pauli_term *terms, int n_terms, int f64);
/* Tr(P rho) on vec(rho) (2n-wire register, ket wires first, complex64); terms name the n system wires.
 * d_out float32 [batch][n_obs]; the same argument checks, 2 * n_qubits <= QMLE_MAX_QUBITS. */
int qmle_density_expval_pauli(const void *d_rho, int n_qubits, int batch, const qmle_pauli_term *terms,
                              int n_terms, int n_obs, float *d_out, qmle_stream stream);
/* Meyer-Wallach: d_out[b] = 2 (1 - 1/n sum_j Tr rho_j^2), Tr rho_j^2 = a^2+d^2+2|c|^2
 * (entanglement.py:86-101 via the Schmidt identity).
 * d_purities (optional, may be NULL): [batch][n] float32 */
int qmle_meyer_wallach(const void *d_states, int n_qubits, int batch, float *d_out,
                       float *d_purities, void *d_workspace, size_t workspace_bytes,
                       qmle_stream stream);
size_t qmle_meyer_wallach_workspace_bytes(int n_qubits, int batch);
/* how many times qmle_meyer_wallach streams the state from HBM at this size (host only;
 * bench.py's bytes-moved accounting): the passes of the tile scheme from 12 qubits on, one
 * cache-resident sweep per wire below */
int qmle_meyer_wallach_reads(int n_qubits);
/* Host only (no GPU needed): what a Meyer-Wallach call decides, as JSON written like qmle_plan_tile_route's (returns
 * the bytes needed, or an error < 0).  plan == NULL: qmle_meyer_wallach on `batch` resident states of `n_qubits`
 * ("route": "standalone").  Otherwise (n_qubits is ignored) the QMLE_MEAS_MEYER_WALLACH epilogue of a batch run of
 * the plan it executes on a chunk of `batch` states: behind the last tile pass ("route": "fused"; `row_shift`: a row
 * of that pass covers 2^row_shift tiles, the "row_shift" of qmle_plan_tile_route for meas 5; QMLE_MW_FUSE_TILED is
 * not read), or on the stored states where that pass cannot report its tile ("route": "resident").  `request_flags`:
 * QMLE_ROUTE_NO_MW_LEAN and QMLE_ROUTE_MW_PER_POSITION (a tiled state's call takes the per-position finish whatever
 * its shape; "total_bytes" does not change with it), nothing else.  Keys: "fusable", "lean" (the first later read reports positions 0..3);
 * "first": the stand-alone first read, or null; "reads": the later reads, in launch order; a read is {"kind":
 * "first" | "later" | "later_low", "lo", "lo2" (its tile: positions 0..3, lo..lo+3, lo2..lo2+3), "q" (2^q tiles per
 * workgroup), "rows" (per state), "stride" (floats per row), "nt" (at least 1 GiB per launch: streamed past the
 * caches)}; "positions"[p]: {"read": the later read that reports position p's cross terms, -1: the first read or the
 * producing pass, "col": its column there}; "finish": "whole-state" | "columns" | "per-position" (fused),
 * "standalone", "per-wire-sweeps" (below 12 qubits); "slices" of the finish; "finish_threads": the block size the
 * fused route's finish launches with (its first kernel; 0 on the other routes); "regions": [{"name", "offset", "bytes",
 * "doubles"}], what the call places in its workspace; "end": the bytes the call checks its workspace against;
 * "total_bytes": what the size query reports for it (>= "end"). */
int qmle_meyer_wallach_describe(const qmle_plan *plan, int n_qubits, int batch, int row_shift, unsigned request_flags,
                                char *buf, size_t cap);
/* Host only, no device work: out[i] = the i-th value of
 * numpy.random.Generator(numpy.random.Philox(key=key)).uniform(low, high, n).astype(float32),
 * bit for bit (Philox4x64-10, numpy's counter and double conventions).  The parameter sampler
 * behind Model.initialize_params -- the reference's jax.random.uniform (model.py:687-693) runs
 * on a threefry stream that cannot be reproduced here; the build's stream is
 * numpy's Philox, and numpy's own loop (~9 ns per value) was two thirds of the wall-clock of
 * Expressibility(12 q, 1024 pairs). */
int qmle_philox_uniform_f32(const uint64_t key[2], uint64_t n, double low, double high, float *out);
/* The same stream written by the GPU into d_out (one work item per Philox block; bit for bit the
 * host version's floats): what utils.uniform uses when a GPU is present. */
int qmle_philox_uniform_f32_device(const uint64_t key[2], uint64_t n, double low, double high,
                                   float *d_out, qmle_stream stream);
/* The same with the key read from DEVICE memory (d_key: two 64-bit words) when the kernel runs: a
 * launch captured in a hipGraph is re-seeded by rewriting those words, not by re-capturing. */
int qmle_philox_uniform_f32_device_key(const uint64_t *d_key, uint64_t n, double low, double high,
                                       float *d_out, qmle_stream stream);
/* numpy.histogram(values, bins=linspace(lo,hi,n_bins+1)) counts (last bin
 * right-inclusive) -- expressibility.py:104-108; d_counts int32[n_bins], zeroed
 * by the call */
int qmle_histogram(const float *d_values, int64_t count, int n_bins, float lo, float hi,
                   int32_t *d_counts, qmle_stream stream);

/* Shot sampling (simulation.py:320-377 sample_shots): for every row of d_probs
 * [batch][2^n] float32 draw `shots` basis states by inverse-CDF sampling (the algorithm of
 * jax.random.choice(key, dim, (shots,), p=probs): r = total * u, first index with
 * cumsum >= r) and histogram them.  u comes from Philox4x32-10 keyed by `seed`, counter =
 * (shot pair, row_offset + row) -- results do not depend on how a batch is chunked or
 * sharded.  d_counts int32 [batch][2^n] (zeroed by the call); d_est_probs (optional, may be
 * NULL) float32 counts / shots.  Workspace: the fp64 CDF. */
int qmle_sample_counts(const float *d_probs, int n_qubits, int batch, int shots, uint64_t seed,
                       uint64_t row_offset, int32_t *d_counts, float *d_est_probs,
                       void *d_workspace, size_t workspace_bytes, qmle_stream stream);
size_t qmle_sample_workspace_bytes(int n_qubits, int batch);
/* sum_i p[b][i] * diag(O_k lifted)[i] for n_obs observables (simulation.py:363-372, the
 * computational-basis estimate Tr(O diag(p))).  HOST arrays: obs_wires = concatenated wire
 * lists, obs_n_wires[k] wires each (first wire = most significant bit of the table index),
 * obs_diag_off[k] = float offset of the 2^k-entry diagonal in the DEVICE array d_diag, or
 * -1 for a Z (x) Z (x) .. parity.  d_out float32 [batch][n_obs]. */
int qmle_probs_diag_expval(const float *d_probs, int n_qubits, int batch,
                           const int32_t *obs_wires, const int32_t *obs_n_wires,
                           const int32_t *obs_diag_off, const float *d_diag, int n_obs,
                           float *d_out, void *d_workspace, size_t workspace_bytes,
                           qmle_stream stream);
size_t qmle_probs_diag_expval_workspace_bytes(int n_obs);

/* ---- adjoint differentiation ---------------------------------------------------------------
 * Gradient of  C = sum_b sum_k weights[b][k] <Z..Z>_k(b)  with respect to every gate angle in
 * ONE backward sweep (what jax.grad through Script.execute gives the reference,
 * tests/test_jaqsi.py:131-141, tests/test_model.py:1097-1145, docs/training.md):
 *   psi = U_N .. U_1 |0>,  lambda = (sum_k w_k Z_k) psi;  for k = N .. 1:
 *   dC/dtheta_k = coef_k Im <lambda| G_k |psi>,  then  psi <- U_k^+ psi,  lambda <- U_k^+ lambda.
 * `fwd` is the ordinary plan of the tape; `rev` is a QMLE_PLAN_NO_FUSION | QMLE_PLAN_NO_ABSORB
 * plan of the REVERSED, DAGGERED tape (one gate per pass), `terms[r]` describes the
 * generator of rev op r:  G = i^n_y X^{x_wires} Z^{z_wires} projected onto |1> on
 * proj_wires (controls), or diag(consts[marks_off + i]) for the Golomb diagonal.
 * d_grad float32 [batch][n_grad_slots] (zeroed by the call); out_slot < 0 = no derivative. */
typedef struct qmle_adjoint_term {
  int32_t out_slot;
  uint32_t x_wires, z_wires, proj_wires; /* bit w = wire w */
  int32_t n_y;
  float coef;
  int32_t marks_off;
} qmle_adjoint_term;
int qmle_adjoint_gradient(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd,
                          const float *d_angles_rev, int batch, const float *d_weights,
                          const uint32_t *obs_wire_masks, int n_obs,
                          const qmle_adjoint_term *terms, int n_terms, float *d_grad,
                          int n_grad_slots, void *d_workspace, size_t workspace_bytes,
                          qmle_stream stream);
size_t qmle_adjoint_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch);
/* The same sweep on the complex128 engine (x64 mode: jax.grad with jax_enable_x64,
 * /root/reference/tests/test_jaqsi.py:57,131-141,764-786): angles, weights and gradients are float64,
 * psi and lambda complex128, one streaming launch per operator (no fusion, like qmle_run_batch_f64).
 * `rev` keeps one source gate per operator (QMLE_PLAN_NO_FUSION or QMLE_PLAN_NO_MERGE); any batch size
 * (samples are processed in rounds of <= 4 GiB of psi + lambda).  d_grad float64 [batch][n_grad_slots]. */
int qmle_adjoint_gradient_f64(qmle_plan *fwd, qmle_plan *rev, const double *d_angles_fwd,
                              const double *d_angles_rev, int batch, const double *d_weights,
                              const uint32_t *obs_wire_masks, int n_obs,
                              const qmle_adjoint_term *terms, int n_terms, double *d_grad,
                              int n_grad_slots, void *d_workspace, size_t workspace_bytes,
                              qmle_stream stream);
size_t qmle_adjoint_workspace_bytes_f64(const qmle_plan *fwd, const qmle_plan *rev, int batch);

/* The same sweeps for observables that are sums of Pauli words (X / Y / Hermitian observables, products, and any
 * number of Z parities as x = 0 words):  C = sum_b sum_o d_weights[b][o] <H_o>(b),  H_o = sum of the `obs_terms`
 * with obs == o.  Only the seed differs: lambda = (sum_t w[b][obs_t] coef_t P_t) psi, by the kernels of
 * qmle_apply_pauli_sum (inside the single launch when the whole sweep runs in LDS).  `obs_terms` is a HOST array
 * with the limits and the argument checks of qmle_apply_pauli_sum (checked first, before any device work; a
 * workspace smaller than the query's answer is QMLE_ERR_INVALID_ARG); everything else, the batch limits
 * included, as for the function each one extends. */
int qmle_adjoint_gradient_pauli(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd,
                                const float *d_angles_rev, int batch, const float *d_weights,
                                const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                                const qmle_adjoint_term *terms, int n_terms, float *d_grad,
                                int n_grad_slots, void *d_ws, size_t ws_bytes, qmle_stream stream);
size_t qmle_adjoint_pauli_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch,
                                          int n_obs_terms, int n_obs);
int qmle_adjoint_gradient_pauli_f64(qmle_plan *fwd, qmle_plan *rev, const double *d_angles_fwd,
                                    const double *d_angles_rev, int batch, const double *d_weights,
                                    const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                                    const qmle_adjoint_term *terms, int n_terms, double *d_grad,
                                    int n_grad_slots, void *d_ws, size_t ws_bytes, qmle_stream stream);
size_t qmle_adjoint_pauli_workspace_bytes_f64(const qmle_plan *fwd, const qmle_plan *rev, int batch,
                                              int n_obs_terms, int n_obs);

/* The same sweeps, also returning MATRIX COTANGENTS: the sensitivity of C to the entries of one-wire matrix gates
 * (QMLE_OP_MAT1, QMLE_OP_MAT1_ROW), from which a caller that knows dU/dtheta forms any dC/dtheta (pulse gates: the
 * Jacobian of the pulse solve).  With lambda_k = lambda with all later gates undone and phi_k = the state in FRONT of
 * the gate at reverse position r on wire q,
 *   G[a][c] = sum_rest conj(lambda_k[a, rest]) phi_k[c, rest]     (a, c = value of wire q),
 *   dC/dtheta = 2 Re sum_ac G[a][c] dU[a][c]/dtheta.
 * One read of psi and lambda gives all eight numbers: the 2x2 moment on the states behind the gate, times the
 * transpose of the reverse op's own matrix U^+.
 *   mat_out[r]  HOST array, one entry per op of `rev` (n_terms of them): index < n_mat of the 2x2 that reverse op r
 *               reports, or -1.  >= 0 on anything but a one-wire matrix operator: QMLE_ERR_UNSUPPORTED (two-wire
 *               matrices are not served); >= n_mat: QMLE_ERR_SLOT_RANGE.
 *   d_cot       [batch][n_mat][2][2][re, im], float / double, zeroed by the call.
 * The seed: exactly one of obs_wire_masks (Z parities, n_obs of them; n_obs_terms ignored) and obs_terms (Pauli
 * words, as for qmle_adjoint_gradient_pauli) is non-NULL, else QMLE_ERR_INVALID_ARG.  d_grad and `terms` as for the
 * functions above: angle gradients and cotangents come from ONE sweep.  The workspace has a query of its own (pass
 * n_obs_terms = 0 for the Z seed); a smaller one is QMLE_ERR_INVALID_ARG.  Routes: the whole sweep in LDS (n <= 13)
 * and one streaming pass per gate serve the request; a `rev` plan compiled for fused tile passes
 * (QMLE_PLAN_NO_MERGE) that does not fit LDS returns QMLE_ERR_UNSUPPORTED -- compile `rev` with
 * QMLE_PLAN_NO_FUSION instead.
 * These two are wrappers of qmle_adjoint_cotangent_at / _f64 below with offsets 8 * index.  NULL and shape errors are
 * QMLE_ERR_INVALID_ARG as before; the codes for mat_out (QMLE_ERR_SLOT_RANGE, QMLE_ERR_UNSUPPORTED) are now decided
 * before the workspace size is looked at; two flagged ops that share one index, which used to overwrite each other,
 * are QMLE_ERR_SLOT_RANGE (overlapping blocks). */
int qmle_adjoint_cotangent(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd, const float *d_angles_rev,
                           int batch, const float *d_weights, const uint32_t *obs_wire_masks,
                           const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                           const qmle_adjoint_term *terms, int n_terms, float *d_grad, int n_grad_slots,
                           const int32_t *mat_out, int n_mat, float *d_cot, void *d_ws, size_t ws_bytes,
                           qmle_stream stream);
size_t qmle_adjoint_cotangent_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch,
                                              int n_obs_terms, int n_obs);
int qmle_adjoint_cotangent_f64(qmle_plan *fwd, qmle_plan *rev, const double *d_angles_fwd,
                               const double *d_angles_rev, int batch, const double *d_weights,
                               const uint32_t *obs_wire_masks, const qmle_pauli_term *obs_terms, int n_obs_terms,
                               int n_obs, const qmle_adjoint_term *terms, int n_terms, double *d_grad,
                               int n_grad_slots, const int32_t *mat_out, int n_mat, double *d_cot, void *d_ws,
                               size_t ws_bytes, qmle_stream stream);
size_t qmle_adjoint_cotangent_workspace_bytes_f64(const qmle_plan *fwd, const qmle_plan *rev, int batch,
                                                  int n_obs_terms, int n_obs);

/* Matrix cotangents of one- AND two-wire matrix gates (QMLE_OP_MAT1 / MAT1_ROW / MAT2 / MAT2_ROW) from the same
 * sweep; the two functions above are thin wrappers of these with offsets 8 * index.  For a gate on wires (w0, w1),
 * in the index convention of its own matrix (row = 2 * value of w0 + value of w1),
 *   M[a][c] = sum_rest conj(lambda[a, rest]) psi[c, rest]   behind the gate,     G = M (U^+)^T,
 *   dC/dtheta = 2 Re sum_ac G[a][c] dU[a][c]/dtheta   with U as the caller passed it: 16 complex numbers from one
 * read of psi and lambda.
 *   cot_off[r]  HOST array, one entry per op of `rev`: offset, in scalars, of reverse op r's block inside a sample's
 *               row of cot_stride scalars, or -1.  A block is 8 scalars ([2][2][re, im]) for a one-wire matrix gate
 *               and 32 ([4][4][re, im]) for a two-wire one.  A block that ends outside the row or overlaps another:
 *               QMLE_ERR_SLOT_RANGE; >= 0 on anything but the four matrix opcodes: QMLE_ERR_UNSUPPORTED; on an op
 *               that was merged into a neighbour or carries a control: QMLE_ERR_INVALID_ARG.  All of this is
 *               checked before any device work.
 *   d_cot       [batch][cot_stride], float / double, zeroed by the call.
 * The workspace queries take `two_wire` != 0 when a two-wire block is requested (16 complex partial sums per block
 * of the streaming route instead of 4).  Routes: the LDS launch (n <= 13) takes the 4x4 moment one row at a time;
 * the streaming route runs one moment kernel over float2 / double2 amplitudes and one finishing kernel; fused tile
 * passes return QMLE_ERR_UNSUPPORTED as above. */
int qmle_adjoint_cotangent_at(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd, const float *d_angles_rev,
                              int batch, const float *d_weights, const uint32_t *obs_wire_masks,
                              const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                              const qmle_adjoint_term *terms, int n_terms, float *d_grad, int n_grad_slots,
                              const int32_t *cot_off, int cot_stride, float *d_cot, void *d_ws, size_t ws_bytes,
                              qmle_stream stream);
size_t qmle_adjoint_cotangent_at_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch,
                                                 int n_obs_terms, int n_obs, int two_wire);
int qmle_adjoint_cotangent_at_f64(qmle_plan *fwd, qmle_plan *rev, const double *d_angles_fwd,
                                  const double *d_angles_rev, int batch, const double *d_weights,
                                  const uint32_t *obs_wire_masks, const qmle_pauli_term *obs_terms, int n_obs_terms,
                                  int n_obs, const qmle_adjoint_term *terms, int n_terms, double *d_grad,
                                  int n_grad_slots, const int32_t *cot_off, int cot_stride, double *d_cot, void *d_ws,
                                  size_t ws_bytes, qmle_stream stream);
size_t qmle_adjoint_cotangent_at_workspace_bytes_f64(const qmle_plan *fwd, const qmle_plan *rev, int batch,
                                                     int n_obs_terms, int n_obs, int two_wire);

/* ---- the adjoint sweep over one segment of a reverse tape, on states the caller holds -------------------------
 * d_pair: DEVICE, [2][batch][2^n] -- psi of every sample, then lambda of every sample -- complex64
 * (qmle_adjoint_segment) or complex128 (_f64), both states as they stand BEHIND the segment.  No forward run and no
 * seed: per op of `rev` (a QMLE_PLAN_NO_FUSION plan of the reversed, daggered segment; any other plan is
 * QMLE_ERR_UNSUPPORTED, as is n < 3) the generator overlap of terms[r] into d_grad[b][out_slot], the one- or two-wire
 * matrix cotangent into d_cot[b][cot_off[r] ..] (cot_off NULL: none; the rules and codes of
 * qmle_adjoint_cotangent_at), then the op on all 2 * batch states.  On return psi and lambda stand in FRONT of the
 * segment.  d_grad [batch][n_grad_slots] and d_cot [batch][cot_stride] are NOT zeroed: only the slots and blocks
 * that the terms name are written, so out_slot may be a column of a whole tape's gradient.  2 * batch <= 65535
 * (QMLE_ERR_INVALID_ARG above).  A workspace smaller than the query's answer (two_wire: a two-wire cotangent is
 * among the request) is QMLE_ERR_WORKSPACE.  All codes are decided before any device work. */
int qmle_adjoint_segment(qmle_plan *rev, const float *d_angles_rev, int batch, void *d_pair,
                         const qmle_adjoint_term *terms, int n_terms, float *d_grad, int n_grad_slots,
                         const int32_t *cot_off, int cot_stride, float *d_cot, void *d_ws, size_t ws_bytes,
                         qmle_stream stream);
size_t qmle_adjoint_segment_workspace_bytes(const qmle_plan *rev, int batch, int two_wire);
int qmle_adjoint_segment_f64(qmle_plan *rev, const double *d_angles_rev, int batch, void *d_pair,
                             const qmle_adjoint_term *terms, int n_terms, double *d_grad, int n_grad_slots,
                             const int32_t *cot_off, int cot_stride, double *d_cot, void *d_ws, size_t ws_bytes,
                             qmle_stream stream);
size_t qmle_adjoint_segment_workspace_bytes_f64(const qmle_plan *rev, int batch, int two_wire);

/* ---- adjoint differentiation of NOISY tapes: one backward sweep over vec(rho) ----------------------------------
 * The tape acts on rho (vec(rho): a 2n-wire register, ket wires 0..n-1, bra wires n..2n-1) as U rho U^+ for a gate and
 * sum K rho K^+ for a channel; C = sum_k w_k Tr(O_k rho).  A channel has no usable inverse, so the forward states are
 * kept and only the observable moves backwards: Lambda_L = sum_k w_k O_k, Lambda_{j-1} = A_j^+ Lambda_j with A_j the
 * doubled operator of tape entry j, and for a gate exp(-i theta G / 2) with rho_j the state behind it
 *   dC/dtheta = Im <lambda_j| G_ket |v_j>,   v = vec(rho), lambda = vec(Lambda), G on the ket wires only.
 * `fwd`: a QMLE_PLAN_NO_FUSION | QMLE_PLAN_TAPE_ORDER plan of the doubled tape (Rot already split into its three
 * rotations), `rev`: such a plan of its reversed, daggered tape; any other plan is QMLE_ERR_UNSUPPORTED.  A STEP names
 * one differentiable source gate: the ops [fwd_first, fwd_first + fwd_count) of `fwd` (its ket operator, its bra
 * operator and the channels behind it on the same wires) and [rev_first, ..) of `rev`, which the call does NOT run
 * through the plans: two kernels apply the gate pair from the sample's angle (column angle_slot of d_angles_fwd) and
 * the channels as ONE superoperator -- d_chan + chan_off: [4][4][re, im] for a one-wire gate, [16][16][re, im] for a
 * two-wire one, DEVICE, in the precision of the call, row index = the step's wires in ASCENDING order, first wire most
 * significant; chan_off = -1: no channel -- to 4 or 16 amplitudes per work item in registers.  Forward, a step reads
 * checkpoint k and writes checkpoint k + 1; backward it reads lambda and checkpoint k, writes lambda and reports
 * term.coef Im i^n_y <lambda'| X^x Z^z Pi_p |v_mid> into d_grad[row][term.out_slot] (`term` as for
 * qmle_adjoint_gradient, wires of the ket half only): five state-sized transfers per step.  Everything outside the
 * steps runs one operator per pass: forward in place on the newest checkpoint, backward on lambda alone.
 * opcode: QMLE_OP_RX / RY / RZ (wires[1] = -1) or CRX / CRY / CRZ / CPHASE / RXX / RYY / RZZ / RZX; steps in tape order.
 * n_cot cotangents per sample: d_weights [n_cot * batch][n_obs], d_angles_rev [n_cot * batch][rev slots] and
 * d_grad [n_cot * batch][n_grad_slots] (zeroed by the call) are sample-minor, row r of lambda reads checkpoint row
 * r % batch; checkpoints are stored once per sample.  n_cot * batch <= 65535.
 * The seed: exactly one of obs_wire_masks (Z parities of the n system wires) and obs_terms (Pauli words of the n
 * system wires with the limits of qmle_apply_pauli_sum, at most 96 of them) is non-NULL, else QMLE_ERR_INVALID_ARG.
 * All codes are decided before any device work: QMLE_ERR_INVALID_ARG also for NULL pointers, 2n < 4, overlapping
 * steps, a generator outside its step's ket wires; QMLE_ERR_WIRE_COUNT / WIRE_RANGE / DUPLICATE_WIRES / SLOT_RANGE for a
 * step's wires and slots; a workspace smaller than the query's answer is QMLE_ERR_WORKSPACE.  The workspace holds
 * (n_steps + 1) * batch checkpoints and n_cot * batch rows of lambda beside the plans' matrix rows. */
typedef struct qmle_density_step {
  int32_t opcode;
  int32_t wires[2];              /* ket wires of the source gate, in the gate's own order */
  int32_t angle_slot;
  int32_t chan_off;              /* offset in scalars into d_chan, or -1 */
  int32_t fwd_first, fwd_count;
  int32_t rev_first, rev_count;
  qmle_adjoint_term term;
} qmle_density_step;
int qmle_adjoint_density(qmle_plan *fwd, qmle_plan *rev, const float *d_angles_fwd, const float *d_angles_rev,
                         int batch, int n_cot, const float *d_weights, const uint32_t *obs_wire_masks,
                         const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                         const qmle_density_step *steps, int n_steps, const float *d_chan, int n_chan, float *d_grad,
                         int n_grad_slots, void *d_ws, size_t ws_bytes, qmle_stream stream);
size_t qmle_adjoint_density_workspace_bytes(const qmle_plan *fwd, const qmle_plan *rev, int batch, int n_cot,
                                            int n_steps);
int qmle_adjoint_density_f64(qmle_plan *fwd, qmle_plan *rev, const double *d_angles_fwd, const double *d_angles_rev,
                             int batch, int n_cot, const double *d_weights, const uint32_t *obs_wire_masks,
                             const qmle_pauli_term *obs_terms, int n_obs_terms, int n_obs,
                             const qmle_density_step *steps, int n_steps, const double *d_chan, int n_chan,
                             double *d_grad, int n_grad_slots, void *d_ws, size_t ws_bytes, qmle_stream stream);
size_t qmle_adjoint_density_workspace_bytes_f64(const qmle_plan *fwd, const qmle_plan *rev, int batch, int n_cot,
                                                int n_steps);
/* host only: the modelled state-sized reads and writes of a call per sample -- forward 1 (checkpoint 0) + 2 per
 * operator outside the steps + 2 per step; backward, times n_cot, 1 (the seed) + 2 per operator behind the tape's
 * first step + 3 per step -- or a negative status for arguments the call would refuse. */
long long qmle_adjoint_density_transfers(const qmle_plan *fwd, const qmle_plan *rev, const qmle_density_step *steps,
                                         int n_steps, int n_cot, int f64);

/* ---- Gram matrices of resident states (quantum geometric tensor) ---------------------------
 * G[g][r][s] = sum_k conj(a[g][r][k]) * b[g][s][k] for g < n_groups, r < rows_a, s < rows_b:
 * d_out complex128, row-major [n_groups][rows_a][rows_b].  Row r of group g starts at amplitude
 * g * group_stride_a + r * 2^n_qubits of d_a (strides in amplitudes).  d_a == d_b with equal rows and
 * strides is the Hermitian case: only the upper block triangle is computed, the rest is its mirror,
 * the diagonal is real.  qmle_gram reads complex64 rows (v_mfma_f32_32x32x2_f32 over sub-slices of
 * 32 amplitudes, each added in fp64); qmle_gram_f64 complex128 rows (fp64 FMA).  Long rows are cut
 * into chunks whose fp64 partials (the workspace; 0 bytes when one chunk covers a row) are added in
 * chunk order: the result is the same bit for bit from call to call.  QMLE_ERR_INVALID_ARG, decided
 * before any device work, for rows outside 1..4096, n_qubits outside 1..30, n_groups outside
 * 1..65535, overlapping groups, complex64 rows not 16-byte aligned, or a workspace smaller than the
 * query's answer. */
int qmle_gram(const void *d_a, const void *d_b, int n_qubits, int n_groups, int rows_a, int rows_b,
              int64_t group_stride_a, int64_t group_stride_b, void *d_out, void *d_ws, size_t ws_bytes,
              qmle_stream stream);
size_t qmle_gram_workspace_bytes(int n_qubits, int n_groups, int rows_a, int rows_b);
int qmle_gram_f64(const void *d_a, const void *d_b, int n_qubits, int n_groups, int rows_a, int rows_b,
                  int64_t group_stride_a, int64_t group_stride_b, void *d_out, void *d_ws, size_t ws_bytes,
                  qmle_stream stream);
size_t qmle_gram_workspace_bytes_f64(int n_qubits, int n_groups, int rows_a, int rows_b);

/* ---- Hamiltonian time evolution (Hermitian.evolve / ParametrizedHamiltonian.evolve) ----------
 * U[r] = the solution at the end of the grid of  dU/dt = -i sum_i f_i(t) H_i U,  U = I at the start, for `rows`
 * independent rows and dim = 2 or 4, on the fixed grid of the reference's commutator-free Magnus integrators
 * (qml_essentials/evolution.py:204-231) with step d_h[r]:
 *   order 2: U <- exp(h A(t_n + h/2)) U, one node per step;
 *   order 4: U <- exp(h (a2 A1 + a1 A2)) exp(h (a1 A1 + a2 A2)) U with A_k = A(t_n + c_k h), c_1,2 = 1/2 -+ sqrt(3)/6,
 *            a_1,2 = 1/4 +- sqrt(3)/6, two nodes per step (c_1 first);
 *   A(t) = -i sum_i c_i(t) H_i.
 * h_terms (HOST): n_terms (1..16) matrices, complex128 row-major; they are taken as Hermitian -- the real diagonal
 * and the entries above it are read.  d_coef: float64 [rows][n_steps * nodes per step][n_terms], the coefficient
 * functions at the node times in node order: the library evaluates no coefficient function, and where a row's grid
 * starts matters to the caller's table alone.  d_h: float64 [rows].  d_out [rows][dim * dim], row-major, complex128
 * (out_f64 = 1) or complex64 (0); the arithmetic is float64 either way.
 * lanes_per_row in {1, 4, 16, 64}: a row's steps are cut into that many contiguous runs, one per lane of a wave; the
 * partial products are multiplied in time order through lane shifts.  The result depends on the split through
 * rounding only.  0: the library chooses (what the second function returns: 1 when the rows alone fill the card,
 * else the widest split that fills it and leaves no lane without a step).
 * The 4x4 exponentials are Taylor series applied to the columns of U, the exponent cut into ceil(norm / 0.5) parts;
 * a row whose h * |sum_i c_i H_i| (largest absolute row sum) exceeds 2^15 or is not finite comes back as NaN.
 * QMLE_ERR_UNSUPPORTED for dim outside {2, 4} or order outside {2, 4}; QMLE_ERR_INVALID_ARG for NULL pointers,
 * n_terms outside 1..16, rows < 1, n_steps < 1, another lanes_per_row, out_f64 outside {0, 1} or rows * lanes
 * beyond 2^31 -- all before any device work. */
int qmle_evolve_magnus(const double *h_terms, int n_terms, int dim, const double *d_coef, const double *d_h, int rows,
                       int order, int n_steps, int lanes_per_row, int out_f64, void *d_out, qmle_stream stream);
int qmle_evolve_lanes(int rows, int n_steps);

/* The same solve with the EXACT derivative of the fixed grid's result in n_dirs (1..64) directions: the scheme is
 * discretised, then differentiated -- neither a finite difference nor a second ODE.  The first arguments are those of
 * qmle_evolve_magnus.  d_dcoef: float64 [rows][n_dirs][n_steps * nodes per step][n_terms], the derivative of the
 * coefficient table in direction k (where a node moves with the direction -- a derivative by an end of the interval --
 * the caller adds f'(t_j) dt_j here: the library evaluates no function).  d_dh: float64 [rows][n_dirs], the derivative
 * of the step.  d_out: complex128 [rows][1 + n_dirs][dim * dim]: slot 0 is U, slot 1 + k its derivative in direction
 * k.  Per exponential factor Omega = h sum_j a_j A(t_j):  dOmega = dh sum_j a_j A(t_j) + h sum_j a_j dA(t_j),
 * U <- E U, dU <- dE U + E dU; dim = 2 in closed form, dim = 4 by the column series with its derivative term by term
 * (the same cut and term count, taken from Omega).  One (row, direction) is one unit of work that recomputes U, so
 * slot 1 + k does not depend on which other directions share the call (bit for bit, at equal lanes_per_row).
 * lanes_per_row as above; at dim = 4 a run of steps takes four lanes (one per column of U), so 64 is refused and
 * 0 never chooses it; 0 chooses qmle_evolve_lanes(rows * n_dirs, n_steps) within that.
 * A row whose norm check fails or whose exponent is not finite comes back NaN in every slot; a direction whose
 * dOmega is not finite comes back NaN in its own slot.
 * The status codes of qmle_evolve_magnus; QMLE_ERR_INVALID_ARG also for NULL d_dcoef / d_dh, n_dirs outside 1..64
 * and rows * n_dirs * lanes beyond 2^31 -- all before any device work. */
int qmle_evolve_magnus_jac(const double *h_terms, int n_terms, int dim, const double *d_coef, const double *d_h,
                           const double *d_dcoef, const double *d_dh, int rows, int n_dirs, int order, int n_steps,
                           int lanes_per_row, void *d_out, qmle_stream stream);

/* qmle_evolve_magnus for dim = 8 and 16 (Hamiltonians on three and four wires): the same grids, node order, float64
 * arithmetic, series cut (ceil(norm / 0.5) parts) and NaN rule (a row whose h * |sum_i c_i H_i|, largest absolute row
 * sum, exceeds 2^15 or is not finite comes back as NaN; its neighbours do not).  d_coef, d_h, rows, order, n_steps as
 * there.  Differences: d_terms is a DEVICE pointer, complex128 [n_terms][dim][dim] row-major, n_terms 1..16 (taken as
 * Hermitian: the real diagonal and the entries above it are read); d_out is complex128 [rows][dim * dim].
 * lanes_per_row: a row's steps are cut into that many contiguous runs; a run takes dim lanes (one per column of U)
 * and a row's runs share a wave, so the allowed values are those with lanes * dim <= 64 -- {1, 4, 8} at dim 8,
 * {1, 4} at dim 16; 0: the library chooses (qmle_evolve_wide_lanes: the widest allowed split that fills the card and
 * leaves every run a step).  The result depends on the split through rounding only.
 * QMLE_ERR_UNSUPPORTED for dim outside {8, 16} (dim 2 and 4: qmle_evolve_magnus; 32 and up are not served) or order
 * outside {2, 4}; QMLE_ERR_INVALID_ARG for NULL pointers, n_terms outside 1..16, rows < 1, n_steps < 1, another
 * lanes_per_row or rows * lanes * dim beyond 2^31 -- all before any device work.  There is no derivative form:
 * gradients through evolved gates on more than two wires are not served. */
int qmle_evolve_magnus_wide(const void *d_terms, int n_terms, int dim, const double *d_coef, const double *d_h, int rows,
                            int order, int n_steps, int lanes_per_row, void *d_out, qmle_stream stream);
int qmle_evolve_wide_lanes(int rows, int n_steps, int dim);

/* ---- pulse-level gates (pulses.PulseGates.RX / RY): every pulse solve of a tape in one launch -----------------------
 * U[s] of dU/dt = -i (cx(t) X + cy(t) Y) U on [0, S], U(0) = I, for n_solves independent 2x2 solves on the fixed
 * Magnus grid described above (order 2 or 4, n_steps equal steps).  d_solves: float64 [n_solves][8], the columns
 * p0, p1, p2, w, T, axis (0 = RX, anything else = RY) and two of padding.  The library evaluates the coefficients
 * itself, at absolute node times, with the envelope centre t_c = t / 2 of the reference (t the running time):
 *   envelope 0 gaussian  A exp(-(t / 2 sigma)^2 / 2)           p = A, sigma
 *            1 square    A while t <= width, else 0            p = A, width
 *            2 cosine    A cos(pi clip(t / (2 width), +-1/2))  p = A, width
 *            3 drag      g (1 - beta (t / 2) / sigma^2), g the gaussian of (A, sigma)   p = A, beta, sigma
 *            4 sech      A / cosh(t / 2 sigma)                 p = A, sigma
 *   mode 0 rwa:   RX (cx, cy) = (env w / 2, 0), RY (0, env w / 2);
 *        1 lab:   cx = env cos(omega_c t + phi) cos(omega_q t) w, cy = -env cos(omega_c t + phi) sin(omega_q t) w,
 *                 phi = 0 (RX) or pi / 2 (RY);
 *        2 drive: the same coefficients through the product-to-sum identities (omega_c -+ omega_q).
 * S is the envelope's support inside the pulse: min(T, width) for square and cosine, T otherwise.
 * d_out [n_solves][4] row-major, complex128 (out_f64 = 1) or complex64 (0); float64 arithmetic either way.
 * d_prev (may be NULL): a result of the same format, normally that of the grid of half the steps; d_err (may be NULL,
 * needs d_prev): float64 [n_solves] <- max over the four entries of |U - U_prev|, NaN when an entry is NaN.
 * lanes_per_solve as lanes_per_row of qmle_evolve_magnus (0: qmle_evolve_lanes(n_solves, n_steps)).  A solve with a
 * step whose |h cx| + |h cy| exceeds 2^15 or is not finite comes back as NaN.
 * QMLE_ERR_UNSUPPORTED for order outside {2, 4}, envelope outside 0..4 or mode outside 0..2; QMLE_ERR_INVALID_ARG for
 * NULL d_solves / d_out, n_solves < 1, n_steps < 1, another lanes_per_solve, out_f64 outside {0, 1}, d_err without
 * d_prev, a frequency that is not finite, or n_solves * lanes beyond 2^31 -- all before any device work. */
int qmle_pulse_unitaries(const double *d_solves, int n_solves, int envelope, int mode, double omega_c, double omega_q,
                         int order, int n_steps, int lanes_per_solve, int out_f64, void *d_out, const void *d_prev,
                         double *d_err, qmle_stream stream);

/* ---- pulse solves with parameter sensitivities (quantum optimal control) ---------------------------------------------
 * The solves of qmle_pulse_unitaries -- same d_solves, envelopes, modes, frequencies, grids and lane split -- together
 * with the EXACT derivative of the fixed-grid Magnus result (discretise, then differentiate: neither a finite
 * difference nor a second ODE).  d_out [n_solves][6][4] row-major complex128:
 *   slot 0 U;  slots 1..5  dU/dp0, dU/dp1, dU/dp2, dU/dw, dU/dT  (the p2 slot is zero for the two-parameter envelopes).
 * Per step U <- E(g) U and dU_k <- dE_k U + E dU_k, E = cos r I - i (sin r / r)(gx X + gy Y), r = |g|, with
 * (cos r - sin r / r) / r^2 from its series for r < 0.05.  The exponents are g = h sum_j a_j c(t_j), h = S / n_steps,
 * t_j = (s + c_j) h, so that besides the envelope's own partial derivatives
 *   d/dw  is the coefficient without its factor w (finite and exact at w = 0);
 *   d/dT  is dh/dT sum_j a_j (c(t_j) + t_j dc/dt(t_j)): the step grows AND the node times move (nothing else depends
 *         on T: the envelope is centred on the running time).
 * Conventions for square and cosine, whose grid ends at S = min(T, width): width < T gives dS/dwidth = 1, dS/dT = 0;
 * otherwise dS/dwidth = 0, dS/dT = 1 -- the tie width == T counts as the T side.  The width derivative therefore has
 * the grid term dh/dwidth sum_j a_j (c + t dc/dt) beside (cosine) the envelope's own.  Square's amplitude is piecewise
 * constant in width; its derivative is taken almost everywhere (zero).
 * A solve with a step whose |gx| + |gy| exceeds 2^15 or is not finite comes back as NaN in all six slots; its
 * neighbours are untouched.  A finite U whose envelope has non-finite partial derivatives keeps its U and gets every
 * slot that reads one of them non-finite: gaussian or sech with sigma = 0 has the envelope 0 at every node, U = I, and
 * 0 x inf for the envelope's derivatives by sigma AND by t, so the p1 slot and the T slot (which carries t dc/dt) are
 * not finite while the p0, p2 and w slots are.  drag with sigma = 0 has 0 x inf in the envelope itself: that solve
 * fails the norm check and is NaN in all six slots.  T = 0, or width = 0 for square, is finite everywhere with U = I.
 * Status codes as qmle_pulse_unitaries: QMLE_ERR_UNSUPPORTED for order outside {2, 4}, envelope outside 0..4 or mode
 * outside 0..2; QMLE_ERR_INVALID_ARG for NULL d_solves / d_out, n_solves < 1, n_steps < 1, another lanes_per_solve, a
 * frequency that is not finite, or n_solves * lanes beyond 2^31 -- all before any device work. */
int qmle_pulse_unitaries_jac(const double *d_solves, int n_solves, int envelope, int mode, double omega_c,
                             double omega_q, int order, int n_steps, int lanes_per_solve, void *d_out,
                             qmle_stream stream);

/* ---- composition of small circuits (quantum optimal control: the evaluator's product rule on the device) ------------
 * Many circuits on 1 or 2 wires (d = 2 or 4) for n_candidates candidates in ONE launch, float64 / complex128.  Per
 * circuit k and candidate c:  U = I, dU_p = 0 (p < n_params), and for every op of the circuit in table order
 *     dU_p <- M dU_p + dM_p U  (every p),   U <- M U.
 * The three structure tables and the row indices are HOST arrays: the library validates every index they hold, then
 * copies them into the caller's device workspace on the stream.  The value pools are DEVICE arrays with their lengths.
 *   qmle_compose_circuit  op_begin..op_end: its ops; n_wires 1 or 2; n_params P_k >= 0; target_off: offset of its
 *       target V_k (d x d row-major) in d_targets, or -1; ov_off / dov_off: where ov[c] and dov[c][p] go in d_ov;
 *       u_off / du_off: where U[c][d][d] and dU[c][p][d][d] go in d_full.  All offsets count complex128 elements.
 *       The output blocks (ov, dov, U, dU of every circuit) must not overlap one another: checked.
 *   qmle_compose_op  kind:
 *       CONST   M from d_mats, no derivative (no terms allowed);
 *       PULSE   M = slot 0 and the derivatives slots 1..5 of row rows[mat_off + c] of d_jac, the result
 *               [n_solves][6][4] of the sensitivity entry point above (mat_off indexes `rows` here; mat_stride unused);
 *       ROT_X / ROT_Y / ROT_Z   M from d_mats, generator derivative (-i/2) sigma M;
 *       CPHASE  M from d_mats (4 x 4), generator derivative i |11><11| M.
 *     For the kinds that read d_mats the matrix of candidate c is at mat_off + c * mat_stride (stride 0: shared).
 *     placement: 0 the wire of a 1-wire circuit; 1 wire 0 of 2; 2 wire 1 of 2; 3 wires [0, 1]; 4 wires [1, 0] (wire 0
 *     is the most significant).  PULSE and ROT_* are 2 x 2 (placements 0..2), CPHASE is 4 x 4 (3, 4), CONST either.
 *     term_begin..term_end: its tangent terms.
 *   qmle_compose_term  the op's derivative by parameter `param` gains d_coefs[coef_off + c] x (slot 1 + `slot` of the
 *       row for PULSE, slot in 0..4 | the generator derivative for ROT_* and CPHASE, slot 0).  Several terms of one op
 *       may name one parameter; a parameter may occur in many ops or in none (its column is then zero).
 * Outputs (either may be NULL, not both):
 *   d_ov    for every circuit with a target, with bit j of column_mask selecting column j:
 *           ov[c] = sum_{j in mask} sum_i conj(V[i][j]) U[i][j], dov[c][p] the same sum over dU_p.  Circuits without a
 *           target write nothing there.
 *   d_full  U and dU of every circuit.
 * One lane per (circuit, candidate, p or "U only", column): columns are summed in a fixed order between neighbouring
 * lanes, no atomics -- results are bit-reproducible and do not depend on n_candidates.  A NaN row of d_jac reaches
 * only the outputs of the (circuit, candidate) pairs that read it.
 * d_workspace: at least what the second function returns, 16-byte aligned.
 * Lifetime of the host tables: they are copied by asynchronous host-to-device copies on `stream`.  From ordinary
 * (pageable) memory the HIP runtime stages the source before the copy call returns, so such tables may be changed or
 * freed as soon as this function returns; the library's own lane table relies on the same property.  Tables in
 * page-locked (hipHostMalloc / registered) memory are read when the stream reaches the copy and must stay unchanged
 * until then.
 * QMLE_ERR_UNSUPPORTED for n_wires outside {1, 2}, an unknown kind or placement; QMLE_ERR_WORKSPACE for a workspace
 * that is missing or too small; QMLE_ERR_INVALID_ARG for NULL tables, n_circuits < 1, n_candidates < 1, both outputs
 * NULL, column_mask without a bit below 4 -- or, with d_ov, without a bit below d of a circuit that has a target --, output
 * blocks that overlap, any op / term / matrix / coefficient / row / target / output range outside its
 * table or pool, a row index >= n_solves, a placement that does not fit the circuit's n_wires or the kind's size, terms on
 * a CONST op, a slot outside the kind's range, param >= n_params, a pool that is needed and NULL, or more than 2^31
 * lanes -- all before any device work. */
enum { QMLE_COMPOSE_CONST = 0, QMLE_COMPOSE_PULSE = 1, QMLE_COMPOSE_ROT_X = 2, QMLE_COMPOSE_ROT_Y = 3,
       QMLE_COMPOSE_ROT_Z = 4, QMLE_COMPOSE_CPHASE = 5 };
typedef struct {
  int32_t op_begin, op_end, n_wires, n_params;
  int64_t target_off, ov_off, dov_off, u_off, du_off;
} qmle_compose_circuit;
typedef struct {
  int32_t kind, placement;
  int64_t mat_off, mat_stride;
  int32_t term_begin, term_end;
} qmle_compose_op;
typedef struct {
  int32_t slot, param;
  int64_t coef_off;
} qmle_compose_term;
int qmle_compose_circuits(const qmle_compose_circuit *circuits, int n_circuits, const qmle_compose_op *ops, int n_ops,
                          const qmle_compose_term *terms, int n_terms, const int32_t *rows, int64_t n_rows,
                          int n_candidates, const void *d_mats, int64_t n_mats, const double *d_coefs, int64_t n_coefs,
                          const void *d_targets, int64_t n_targets, const void *d_jac, int n_solves,
                          unsigned column_mask, void *d_ov, int64_t ov_len, void *d_full, int64_t full_len,
                          void *d_workspace, size_t workspace_bytes, qmle_stream stream);
size_t qmle_compose_workspace_bytes(int n_circuits, int n_ops, int n_terms, int64_t n_rows);

/* ---- analytic Fourier coefficients: the sine-cosine tree of a Pauli-rotation circuit, merged into a DAG -------------
 * (coefficients.FourierTree.)  Node j stands for a bare Pauli word in front of the rotations 0..k of the canonical
 * circuit, k its LEVEL.  Its value V_j is a function on the frequency grid: dims[0] x .. x dims[n_axes - 1] points,
 * every dims[a] odd, axis 0 slowest, F their product; the point with coordinates (g_0, ..) is the frequency vector
 * omega_a = g_a - (dims[a] - 1) / 2.  n_axes = 0 is the grid of the single point omega = () (F = 1): plain numbers.
 * A child slot holds a node index >= 0, QMLE_FOURIER_ONE (the function that is 1 at omega = 0 and 0 elsewhere: a
 * diagonal word in front of no rotation) or QMLE_FOURIER_ZERO (the zero function).  With a = V[cos_child],
 * b = V[sin_child] and p = power (0..3) the value of a node on level k is, for every sample,
 *     kind QMLE_FOURIER_ANGLE   V = cos(t) a + i^(1+p) sin(t) b,         t = d_angles[sample][column]
 *     kind QMLE_FOURIER_SHIFT   V = (T+ a + T- a) / 2 + i^p (T+ b - T- b) / 2
 * where (T+ f)(omega) = f(omega - shift e_axis), (T- f)(omega) = f(omega + shift e_axis), and f is 0 outside the grid:
 * the second line is the first with t = shift x_axis, written in the coefficients of e^{i omega x}.  The result is
 *     d_out[sample][r][g] = i^root_phase[r] V[roots[r]][g],     complex128, [batch][n_roots][F].
 *   qmle_fourier_node   cos_child, sin_child, power, and a pad that is not read.
 *   qmle_fourier_level  node_begin..node_end: the nodes of the level; kind; column (ANGLE) or axis and shift (SHIFT,
 *       shift a signed integer != 0).  The levels are in circuit order and tile the node table: level 0 begins at
 *       node 0, every level begins where the one before it ends (a level may be empty), the last ends at n_nodes.
 *       Every child of a node lies on a lower level.  n_levels = 0 with n_nodes = 0 is allowed (the roots are
 *       terminals then).
 * The node, level, root and dims tables are HOST arrays: the library checks every index in them and copies them into
 * the workspace on the stream (lifetime as for qmle_compose_circuits).  d_angles is a DEVICE array [batch][n_columns]
 * of float64; sin and cos are evaluated on the device, in float64 like everything else.
 * One workgroup per sample walks the levels in order with a workgroup barrier between them; its lanes are spread over
 * (node, grid point) of the level.  Every value has one writer and every sum a fixed order: no atomics, the output of
 * a call is bit-reproducible and does not depend on batch.  The values of a sample live in its slice of the workspace,
 * n_nodes x F complex128: a call with one sample and a large DAG runs on one compute unit.
 * d_workspace: at least what the second function returns, 16-byte aligned.
 * QMLE_ERR_WORKSPACE for a workspace that is missing, misaligned or too small; QMLE_ERR_UNSUPPORTED for an unknown
 * kind or n_axes outside 0..QMLE_FOURIER_MAX_AXES; QMLE_ERR_INVALID_ARG for a NULL table that is needed, batch < 1,
 * n_roots < 1, n_nodes or n_levels < 0, an even or non-positive dims entry, F or a level's (nodes x F) at or beyond
 * 2^31, levels that do not tile the node table, a child or root that is neither a terminal code nor a node index below
 * the level's node_begin (below n_nodes for a root), a power or root phase outside 0..3, a column outside
 * 0..n_columns-1, an axis outside 0..n_axes-1, a shift that is 0 or whose magnitude reaches dims[axis], NULL d_angles
 * while a level reads a column, or NULL d_out -- all before any device work. */
enum { QMLE_FOURIER_ONE = -1, QMLE_FOURIER_ZERO = -2 };
enum { QMLE_FOURIER_ANGLE = 0, QMLE_FOURIER_SHIFT = 1 };
#define QMLE_FOURIER_MAX_AXES 8
typedef struct {
  int32_t cos_child, sin_child, power, pad;
} qmle_fourier_node;
typedef struct {
  int32_t node_begin, node_end, kind, column, axis, shift;
} qmle_fourier_level;
int qmle_fourier_dag(const qmle_fourier_node *nodes, int n_nodes, const qmle_fourier_level *levels, int n_levels,
                     const int32_t *roots, const int32_t *root_phase, int n_roots, const int32_t *dims, int n_axes,
                     const double *d_angles, int n_columns, int batch, void *d_out, void *d_workspace,
                     size_t workspace_bytes, qmle_stream stream);
size_t qmle_fourier_workspace_bytes(int n_nodes, int n_levels, int n_roots, int64_t grid_points, int batch);

#ifdef __cplusplus
}
#endif
#endif /* QMLE_SV_H */
