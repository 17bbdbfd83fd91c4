// Host-side interfaces between the translation units of libqmle_sv (not part of the ABI):
//   qmle_engine.hip    plan objects on the device, angle / matrix builders, qmle_run_batch & co.: the layout
//                      of its workspace (BatchLayout), the two-stream chunk pipeline (ChunkPipeline)
//   qmle_tile.hip      LDS-tile passes (k_tile, k_tile2, k_reg_measure*, product passes)
//   qmle_direct.hip    streaming passes (one gate in place, the Golomb diagonal, fills)
//   qmle_analysis.hip  measurement / analysis kernels of resident states, samplers
//   qmle_mw.hip        Meyer-Wallach: read kernels of resident states, the sums behind a producing tile pass, and
//                      their host path (one plan of the reads, one workspace layout per route, three finishes)
//   qmle_adjoint.hip   adjoint differentiation in complex64: one check, one route choice, three routes (LDS, fused
//                      tile passes, one streaming pass per gate); the stage loop of the last two on states the
//                      caller holds (qmle_adjoint_segment)
//   qmle_f64.hip       complex128 engine (its own matrix builder and constants) and its adjoint sweep
//   qmle_adjoint_dev.h what those two sweeps share: the kernels that are one text in both precisions, a sweep's
//                      arguments and their checks, the launch pairs of the per-gate sweep, the bodies of the
//                      extern "C" entry points (qmle_wide.hip takes cot_finish_entry from it, nobody else includes it)
//   qmle_density_dev.h the adjoint sweep of a NOISY tape over vec(rho) (qmle_adjoint_density / _f64), one text for those
//                      two units: the step kernels, the seeds, the checks, the walk of the two plans
//   qmle_wide.hip      the matrix cotangent of a dense gate on three or four wires (qmle_wide_moment): the moment of
//                      psi and lambda on the matrix cores, per-block partials, one finishing kernel
//   qmle_density_wide.hip  Kraus maps on three or four system wires of a resident vec(rho) (qmle_density_apply_wide):
//                      wide gates and wide channels of a noisy tape, a 12-position LDS tile, two forms on the matrix cores
//   qmle_gram.hip      Gram matrices of resident states
//   qmle_evolve.hip    Hamiltonian time evolution: 2x2 / 4x4 propagators on the fixed Magnus grids (qmle_evolve_magnus)
//                      the pulse solves with and without sensitivities, and the composition of small circuits
//                      from them (qmle_compose_circuits)
//   qmle_fourier.hip   analytic Fourier coefficients: the merged sine-cosine DAG of a Pauli-rotation circuit walked
//                      level by level, one workgroup per parameter set (qmle_fourier_dag)
//   qmle_pauli.hip     Pauli-word observables of resident states and of vec(rho), their host planner; applying a
//                      weighted sum of words to resident states (the seed of the adjoint sweep)
// Kernels stay private to their unit (anonymous namespaces); what crosses a unit boundary is a
// plain host function that launches them.  The host idioms every unit needs live here (wire masks ->
// position masks and their range check, aligning a caller's workspace, FNV-1a); align_up, grid_for and
// kMaxGridY sit in qmle_dev.h.
//
// Environment switches: the library reads these ten and no others (tests/test_abi_cpu.py).  Unset,
// each one leaves the measured default in place.
//   QMLE_NO_CHUNK_OVERLAP=1  batch chunks run on the caller's stream alone instead of alternating
//                            between two internal streams.  Read per call.  bench.py (k2_one_stream,
//                            k2_three_pass), tests.
//   QMLE_MW_FUSE_TILED=0     Meyer-Wallach of a tiled state: the stand-alone reads instead of the sums
//                            of the producing pass.  Read per call.  bench.py, tests.
//   QMLE_NO_TOP_FIRST=1      no schedule candidate whose first tile sits on the top positions.  Read
//                            per plan compile.  bench.py (k2_three_pass), tests.
//   QMLE_FORCE_CAND=<k>      run schedule candidate k instead of the pass-cost model's choice.  Read per
//                            plan compile.  tests, tools/cand_sweep.py.
//   QMLE_PAD_HIGH=<1 | p>    pad the last stage's tile from the top positions (p >= 2: position p
//                            first).  Read per plan compile.  tests.
//   QMLE_NO_MULTI_ZIN=1      k_tile2 keeps one tile per workgroup when the tile has known-zero local
//                            bits.  Read per launch.  tests.
//   QMLE_K1_CTRL_BURST=<p>   controlled direct passes take 4-row bursts from target position p on (0:
//                            never).  Read per launch.  tests.
//   QMLE_MW_NO_LEAN=1        the producing pass reports Meyer-Wallach positions 0..3 itself instead of
//                            the first later read.  Read per call.  tests.
//   QMLE_MW_FINISH_PER_POSITION=1  a fused Meyer-Wallach call on a tiled state takes the per-position finish
//                            whatever its shape (unset: only where the rows are too wide for the columns
//                            finish); whole-state plans ignore it.
//                            Read per call.  tests.
//   QMLE_RNG_THREADS=<k>     host threads of the Philox parameter sampler (qmle_rng.cpp).  Read per
//                            call.  Shared hosts.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "qmle_internal.h"

namespace qmle {

// Which column of a 33-float partial row an observable reads, and the sign of row i:
// (-1)^popcount(row_mask[k] & i) -- observables that are Z on ONE position of the last tile times
// Z's on outer positions (bits of the tile index).
struct ObsBits {
  int8_t bits[QMLE_MAX_QUBITS] = {};
  uint32_t row_mask[QMLE_MAX_QUBITS] = {};
};

// what a tile pass does with the finished tile (launch_tile's `meas`)
enum TileMeas : int {
  TM_STORE = 0,   // write the tile back into the state buffer
  TM_PROBS = 1,   // write |psi|^2 to out (float)
  TM_EXPVAL = 2,  // whole-state only: <Z> on obs bits
  TM_EXPVAL_PARTIAL = 3,  // last pass of a tiled state: per-tile signed sums for EVERY bit
                          // -> out[b][tile][33] (k_expval_final reduces); state not stored
  TM_EXPVAL_MASKS = 4,    // same, for Z-parity observables (obs_mask): per-tile Walsh-Hadamard
                          // transform of |psi|^2 -> out[b][tile][k < n_obs]
  TM_STORE_MW = 5,        // TM_STORE + the tile's Meyer-Wallach sums -> out[b][tile][kMwFusedRow] (tile_mw_row)
  TM_MW_ONLY = 6,         // whole-state tiles: the Meyer-Wallach row alone, no state is stored
};

struct ProfScope {  // records a start/stop event pair around one stage launch
  qmle_plan *p;
  hipStream_t stream;
  size_t slot;
  bool active;
  ProfScope(qmle_plan *plan, int stage_idx, hipStream_t s) : p(plan), stream(s), slot(0), active(false) {
    StageProfile &pr = plan->prof;
    if (pr.on && pr.used < pr.start.size()) {
      slot = pr.used++;
      pr.stage[slot] = stage_idx;
      active = hipEventRecord((hipEvent_t)pr.start[slot], stream) == hipSuccess;
    }
  }
  ~ProfScope() {
    if (active) (void)hipEventRecord((hipEvent_t)p->prof.stop[slot], stream);
  }
};

// ---- host idioms every unit shares ----
// wires (bit w = wire w) -> bit positions of the state index (wire w is position n - 1 - w)
inline uint32_t wires_to_pos(uint32_t wires, int n) {
  uint32_t m = 0;
  for (int w = 0; w < n; ++w)
    if (wires & (1u << w)) m |= 1u << (n - 1 - w);
  return m;
}
// a product of Z's / a generator's support: at least one wire and none beyond the register; otherwise
// QMLE_ERR_WIRE_RANGE.  (At n = 32 every bit is a wire, and a shift by n would be undefined.)
inline bool valid_wire_mask(uint32_t wires, int n) { return wires != 0 && (n >= 32 || !(wires >> n)); }
// The caller's workspace from its first 256-byte boundary on: moves `ws` there and takes the skipped bytes
// off `bytes`.  false: the workspace ends before that boundary.
inline bool align_workspace(char *&ws, size_t &bytes) {
  const size_t mis = (size_t)(256 - ((uintptr_t)ws & 255)) & 255;
  if (bytes < mis) return false;
  ws += mis;
  bytes -= mis;
  return true;
}
// At least 1 GiB per launch streams past the caches: `states` states of n qubits, 8 bytes an amplitude.
inline bool launch_streams_past_caches(uint64_t states, int n) { return (states << (n + 3)) >= (1ull << 30); }
// FNV-1a over a byte range; `h`: the hash so far, to run several ranges into one value
inline uint64_t fnv1a(const void *data, size_t bytes, uint64_t h = 1469598103934665603ull) {
  const unsigned char *c = (const unsigned char *)data;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ c[i]) * 1099511628211ull;
  return h;
}

// ---- qmle_engine.hip ----
int ensure_device_plan(qmle_plan *p);
bool plan_sparse(const qmle_plan *p);  // known-zero tracking is on for runs of this plan
size_t ws_mats_bytes(const qmle_plan *p, int batch);
size_t workspace_bytes_one(const qmle_plan *plan, int batch, int meas_type, int states_in_flight);
// forward_only: just the matrices the forward tile / direct kernels read (qmle_plan::n_groups_needed)
// measured_from: measured_records_from(p, meas_type) of a batch run; every other caller keeps the phase-exact records
int launch_build_matrices(const qmle_plan *p, const float *d_angles, float *d_mats, int batch, hipStream_t stream,
                          bool forward_only = false, uint32_t measured_from = 0xffffffffu);
// Where in the matrix row the records start that a run of `p` with this measurement builds in measured mode (DESIGN
// 9n): the product-form records of its last stage, when that stage is a tile stage with closing-free groups and the run
// ends it in |amplitude|^2 only -- QMLE_MEAS_EXPVAL_Z, which is also what the Z-parity entries run as -- and for nothing
// else; 0xffffffff: none.  A function of the plan and the measurement alone (no HIP call, no environment).
uint32_t measured_records_from(const qmle_plan *p, int meas_type);
int run_batch_masks(qmle_plan *plan, const float *d_angles, int batch, int meas_type,
                    const uint32_t *obs_masks, int n_obs, void *d_out, void *d_workspace,
                    size_t workspace_bytes, hipStream_t stream, uint64_t *ws_token = nullptr);
int run_stage_inplace(qmle_plan *plan, const Stage &st, float2 *d_states, const float *d_mats,
                      const float *d_angles, int batch, hipStream_t stream);

// ---- qmle_tile.hip ----
size_t tile_lds_bytes(int T, int L, int n_slots);
int tile_threads(int T);
// walk flags of k_tile2 (Tile2Args::walk)
constexpr uint32_t kWalkSlab = 1u, kWalkSyncStaged = 2u, kWalkSyncTileEnd = 4u, kWalkDma = 8u, kWalkLaneSwap = 16u,
                   kWalkLaneSwapCross = 32u;
// What the caller of a tile pass knows (route_tile's input beside the plan).
struct TileRequest {
  int batch = 1;
  bool init_zero = false;   // the pass starts from |0..0> instead of reading the states
  int meas = TM_STORE;      // TileMeas
  int n_obs = 0;
  bool from_zero = false;   // the run started from |0..0>: Stage::zero_in holds (with known-zero tracking on)
  bool fold_cols = false;   // the fold-column buffer is there (product passes)
  bool multi_rows = false;  // the caller takes partial rows that cover several tiles (TileRoute::row_shift)
  int zeroed_states = 0;    // a filled first pass: that many states of the buffer already hold zeros outside tile 0
  bool semi_single = false; // the observables meet the last tile in at most one position each (classify_observables)
  bool no_multi_zin = false;  // QMLE_NO_MULTI_ZIN is set
  bool no_mw_lean = false;    // QMLE_MW_NO_LEAN is set
};
// How a tile stage runs: everything launch_tile decides, as a value.  route_tile computes it from the plan and the
// request alone (no HIP call, no environment, no global state, no allocation); launch_tile issues it.
struct TileRoute {
  int status = QMLE_OK;     // != QMLE_OK: the request is refused and nothing is launched
  TileFamily family = TF_TILE;
  // instantiation (the template parameters the family has)
  bool dense4 = false, mw = false;                                 // k_tile; mw: k_tile2 as well
  bool measure = false, multi = false, ws = false, masks = false;  // k_tile2
  int mono_q = 0;                                                  // k_reg_measure_mono: Q, PAIR
  bool pair = false;
  bool nt = false;  // non-temporal policy: TileArgs::nt (k_tile, k_tile2 -- there also the NT parameter --,
                    // k_tile_product), the NT parameter of k_product_stream and k_reg_measure_mono
  // launch shape
  unsigned grid_x = 1, grid_y = 1, threads = 64;
  size_t lds_bytes = 0;
  // TileArgs fields beside nt
  bool compact = false;
  uint32_t tile_free = 0;
  bool mw_lean = false, slots_in_lds = false;
  // a zero fill of the states precedes the launch / would have, but the zeros are in place (TileRequest::zeroed_states)
  bool fill = false, fill_elided = false;
  // rows and walk: tiles per workgroup; a partial row covers 2^row_shift tiles (the tile walk and k_reg_measure*)
  int tpw = 1, row_shift = 0;
  uint32_t walk = 0;  // kWalk* (k_tile2)
  // <Z> from the last group's registers; ... in a tile loop without a workgroup barrier; product-form groups run
  bool from_regs = false, wave_private = false, product_form = false;
  // the DMA walk with the last group through lane swaps runs in k_measure_walk: every group in product form, none that
  // scatters re-layouts, 1..3 gathered groups, swaps straight or crossed (family, instantiation fields, launch shape and rows stay k_tile2's)
  bool walk_kernel = false;
};
TileRoute route_tile(const qmle_plan *p, size_t stage, const TileRequest &rq);
// the device pointers of a tile pass
struct TileBuffers {
  float2 *states = nullptr;
  const float *mats = nullptr, *angles = nullptr;
  void *out = nullptr;
  const uint32_t *obs_masks = nullptr;
  float2 *cols = nullptr;  // fold columns (TileRequest::fold_cols)
  float *coef = nullptr;   // k_mono_coef's rows (k_reg_measure_mono)
};
// Route, then issue: first-use setup, the optional fill and the kernel of route_tile(p, stage, rq).  `rq`'s two
// switches are read here, per launch.  *taken: the route (also when it was refused).
int launch_tile(const qmle_plan *p, size_t stage, const TileBuffers &b, TileRequest rq, hipStream_t stream,
                TileRoute *taken = nullptr);

// ---- qmle_direct.hip ----
int launch_direct(const qmle_plan *p, const LoweredOp &op, float2 *states, const float *mats,
                  int batch, hipStream_t stream);
void launch_init_zero(float2 *states, int n, int batch, hipStream_t stream);   // |0..0> per state
void launch_diag_all(float2 *states, int n, int batch, const float *marks, const float *angles,
                     int n_slots, int slot, hipStream_t stream);
void launch_fill_zero(float2 *states, uint64_t n_float4, hipStream_t stream);

// ---- qmle_analysis.hip ----
int expval_blocks(int n);
int overlap_blocks(int n);
int run_expval(const float2 *states, int n, int batch, const int8_t *obs_bits, int n_obs,
               float *d_out, void *ws, size_t ws_bytes, hipStream_t stream);
int run_parity_pos(const float2 *states, int n, int batch, const uint32_t *pos_masks, int n_obs,
                   float *d_out, void *ws, size_t ws_bytes, hipStream_t stream);
void launch_expval_final(const float *partial, int n_rows, int batch, int n_obs, const ObsBits &ob,
                         float *d_out, hipStream_t stream);
void launch_probs(const float2 *states, float *d_out, uint64_t total_chunks, hipStream_t stream);
void launch_density(const float2 *states, float2 *d_out, int n, int batch, hipStream_t stream);

// ---- qmle_mw.hip ----
// Meyer-Wallach behind the pass that produced the state (QMLE_MEAS_MEYER_WALLACH): `last` left one
// row per tile at the start of `ws` (TM_STORE_MW / TM_MW_ONLY); d_out [batch][n + 1] = (Q, purities by wire)
bool mw_fusable(int n, const Stage &last);
// tiled state: the producing pass leaves the cross terms of positions 0..3 to the first later read (TileArgs::mw_lean)
// (mw_lean_layout: what the stage allows; mw_no_lean_switch: QMLE_MW_NO_LEAN is set; mw_lean: both)
bool mw_lean(int n, const Stage &last);
bool mw_lean_layout(int n, const Stage &last);
bool mw_no_lean_switch();
size_t mw_fused_ws_bytes(int n, int batch, const Stage &last);
// (a row covers 2^row_shift tiles; *finish_run, when given: the MwFinish the call queued, for LastRun::mw_finish)
int run_mw_fused(const float2 *states, int n, int batch, const Stage &last, int row_shift, void *ws,
                 size_t ws_bytes, float *d_out, hipStream_t stream, int *finish_run = nullptr);
size_t mw_resident_ws_bytes(int n, int batch);
int run_mw_resident(const float2 *states, int n, int batch, void *ws, size_t ws_bytes, float *d_out,
                    hipStream_t stream);

// ---- qmle_pauli.hip ----
// lambda = (sum_t weights[b][terms[t].obs] * terms[t].coef * P_t) psi_b, the seed of the adjoint sweep for observables
// that are sums of Pauli words.  pauli_seed_begin merges the terms into unique words and puts the word tables and
// the CSR of their terms into the workspace (pauli_seed_ws_bytes; sized for at most `max_batch` states per
// pauli_seed_apply / pauli_seed_flat); complex128 states and float64 weights with f64.  `flat`: the table is one
// PauliWordDev per word (what k_adjoint_lds walks) and only pauli_seed_flat may follow -- it computes the
// coefficient rows coef[b][word] of `batch` samples and hands out both tables.
struct PauliSeed;
struct PauliWordDev {
  uint32_t x, z;  // bit positions
  int32_t im;     // ny odd: the phase left beside the coefficient is -i, else 1
  int32_t pad;
};
int pauli_seed_check(int n_qubits, const qmle_pauli_term *terms, int n_terms, int n_obs);
size_t pauli_seed_ws_bytes(int batch, int n_terms, bool f64);
int pauli_seed_begin(PauliSeed **out, int n, int max_batch, const qmle_pauli_term *terms, int n_terms, int n_obs,
                     bool f64, bool flat, void *d_ws, size_t ws_bytes, hipStream_t stream);
int pauli_seed_apply(const PauliSeed *sd, const void *d_psi, void *d_lam, int batch, const void *d_weights,
                     hipStream_t stream);
int pauli_seed_flat(const PauliSeed *sd, int batch, const float *d_weights, hipStream_t stream,
                    const PauliWordDev **d_words, const float **d_coef, int *n_words);
void pauli_seed_end(PauliSeed *sd);

}  // namespace qmle
