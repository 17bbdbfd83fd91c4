// Internal structures shared by the host-side plan compiler (qmle_plan.cpp) and
// the gfx950 kernels / C-ABI entry points (the qmle_*.hip units, see qmle_host.h).  Not part of the ABI.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "qmle_sv.h"

namespace qmle {

// All kernels work in "bit position" space: wire w of an n-qubit register is bit
// p = n-1-w of the flat amplitude index (wire 0 = MSB, simulation.py:100-104).

enum LKind : uint8_t {
  LK_1Q = 0,       // (0..2 controls) x dense/diagonal 2x2 on t0
  LK_2Q = 1,       // (0..1 controls) x dense 4x4 on (t0,t1); row = 2*bit[t0] + bit[t1]
  LK_DIAG_ALL = 2, // full-register diagonal exp(-i * mark[i] * x)
  LK_4Q = 3        // dense 16x16 on (t0, t1, c0, c1) = 4 TARGET bits in wire order (MSB first);
                   // batch-constant matrix in the const blob (2-qubit Kraus superoperators)
};
enum LFlag : uint8_t {
  LF_DIAG = 1,     // matrix is diagonal
  LF_PERMX = 2,    // matrix is exactly Pauli-X (CX / CCX / X): a pure swap of amplitudes
  LF_PHASE = 4,    // diagonal with m00 == 1 exactly (CZ, ControlledPhaseShift): only target = 1 changes
};

// A run of ops applied in ONE LDS round trip: every thread gathers the 2^4 amplitudes
// spanned by `bits` into registers, applies all ops of the group there, scatters back.
enum GKind : uint8_t {
  GK_SWEEP = 0,   // one op, LDS sweep
  GK_REG4 = 1,    // run of (controlled) 2x2 ops on <= 4 bits, in registers
  GK_DENSE4 = 2,  // one LK_4Q op: gather over its 4 bits, 16x16 matrix-vector product
  GK_REG4X = 3    // a GK_REG4 run that also holds uncontrolled LK_2Q ops (dense 4x4 on two of the group's bits:
                  // the 1-wire Kraus superoperators of vec(rho), RXX ...); t0 / t1 are GROUP-local too.  Only the
                  // DENSE4 instantiations of the tile kernels run it (the common ones keep their register budget)
};
struct OpGroup {
  uint8_t kind;
  uint8_t n_ops;
  uint8_t bits[4];    // GK_REG4: tile-local bit positions, ascending
  uint8_t pad[2];
  uint32_t op_begin;  // first op (index into the plan's dev_ops); ops of a GK_REG4
                      // group carry GROUP-local bit indices 0..3 in t0 / c0
  uint32_t pad2;
};
static_assert(sizeof(OpGroup) == 16, "OpGroup layout");

// Device-visible lowered operation (16 bytes).
struct LoweredOp {
  uint8_t kind;
  uint8_t flags;
  int8_t t0, t1;     // target bit positions (t1 = -1 for LK_1Q)
  int8_t c0, c1;     // control bit positions or -1
  uint8_t nc;        // number of controls
  uint8_t pad;
  uint32_t mat_off;  // LK_1Q/LK_2Q: float offset in the per-sample matrix row
                     // LK_DIAG_ALL: float offset of the marks in the const blob
  int32_t slot;      // LK_DIAG_ALL: angle-table column, else -1
};
static_assert(sizeof(LoweredOp) == 16, "LoweredOp layout");

// One source gate feeding the per-sample matrix builder (24 bytes).
struct BuildOp {
  uint16_t opcode;
  uint16_t pad;       // inside a dim-4 group: 0 = a 4x4 source, 1 / 2 = a 2x2 source on the pair's first / second wire
  int32_t slot[3];
  int32_t const_off;
  uint32_t pad2;
};
static_assert(sizeof(BuildOp) == 24, "BuildOp layout");

// A matrix = product of build ops [begin,end) in tape order (later gate on the left).
// dim = kBuildChain: a chain of unit-pivot records (build_matrices_body).  [begin, end) then holds the source gates of
// the chain's members in stream order, each member closed by a marker (opcode kChainMark, pad = ChainMember,
// const_off = float offset of the member's record in the matrix row); the last member is the carrier.
struct BuildGroup {
  uint32_t begin, end;
  uint32_t mat_off;
  uint32_t dim;  // 2 or 4; kBuildChain
};
// dim = kBuildProduct: the product-form record of one Group2 (assign_product_forms; qmle_matrices.h, product_form_group).
// [begin, end) holds the source gates of the group's members in stream order, each closed by a marker as in a chain:
// pad = what the op's ops2 record holds (ChainMember; CM_PLAIN: the operator itself), const_off = the member's
// in-thread bit -- or -1 for a unit-form member of the carrier's chain that sits in an earlier group: its pivot enters
// P, nothing else.  mat_off = float offset of the record (kProductRecFloats floats) in the matrix row.  The markers of a
// group with kGroupClosingFree carry pad2 = 1: the builder may write the record in measured mode.
constexpr uint32_t kBuildChain = 1, kBuildProduct = 3;
constexpr uint16_t kChainMark = 0xffffu;
enum ChainMember : uint16_t { CM_UNIT_DENSE = 0, CM_UNIT_DIAG = 1, CM_CARRIER = 2, CM_PLAIN = 3 };
// Product-form record, in floats: [0, 32) the opening diagonal (16 complex, entry 0 = 1), [32, 40) per in-thread bit
// the pair (-t, u) of the direct real step or (t', 0) of the mirrored one, [40, 44) per in-thread bit the form word --
// the float 0 (no member on that bit), 1 (direct) or 2 (mirrored) --, [48, 80) the closing diagonal (16 complex).
// Measured mode (product_form_group): the pair is (-tau, s) of the three-shear rotation, the form word the
// float 3, the closing diagonal exact ones, and float 44 (kProductRecNoClose) the float 1: "no closing diagonal" -- 0
// in every other record.  The record alone tells the kernel which mode it is in.
constexpr uint32_t kProductRecFloats = 80, kProductRecSteps = 32, kProductRecForms = 40, kProductRecClose = 48;
constexpr uint32_t kProductRecNoClose = 44;
constexpr int kMaxChainUnits = 32;  // unit-form ops per chain: |1 / pivot| <= sqrt 2, so a state is scaled by <= 2^16

// ---- fast tile path (k_tile2) ---------------------------------------------------------------
// A register-tile group whose LDS addressing is a host-built table: thread t gathers its 16
// amplitudes from byte addresses tbl[t] ^ off[c] (XOR-swizzle and the x8 already folded in).
// Basis permutations (X, CX: GF(2)-affine index maps) between groups never move data: they
// change the logical -> physical layout map the tables are built from.  `relayout` groups
// scatter to the identity layout (tbl2 / off2) behind an extra barrier: the last group of a
// stage does, so that the store / measure epilogue indexes the tile plainly.
// Ops of a group carry group-local bits (t0, c0 in 0..3) and a dispatch code in `pad`.
enum FastCode : uint8_t {
  FC_DENSE = 0,     // + tb                      dense 2x2 on bit tb
  FC_CDENSE = 4,    // + 3 * cb + (tb - (tb>cb)) controlled dense 2x2
  FC_DIAG = 16,     // + tb
  FC_CDIAG = 20,    // + 3 * cb + ..
  FC_X = 32,        // + tb                      in-register Pauli-X (pairs swapped)
  FC_CX = 36,       // + 3 * cb + ..             in-register CX
  // unit-pivot forms (assign_unit_forms, qmle_plan.cpp): the record holds U / pivot, the pivots of a stage's chain
  // are multiplied into its carrier gate
  FC_UDENSE = 48,   // + tb                      [[1, x], [y, z]] or [[x, 1], [y, z]] (the record's form word says which)
  FC_UDIAG = 52,    // + tb                      diag(1, m11 / m00)
  FC_COUNT = 56
};
struct Group2 {
  uint32_t op_begin;   // first op in qmle_plan::ops2
  uint16_t n_ops;
  uint8_t relayout;
  uint8_t sync;        // bit 0: the measuring walk needs a workgroup barrier in front of this group's gather (Stage::fast_info)
                       // bit 1 (kGroupProduct): the group runs in product form, its record at prod_off
                       // bit 2 (kGroupProductLow1): ... and no member sits on in-thread bit 0 or 1 (opening entries 0..3 are 1)
                       // bit 3 (kGroupClosingFree): ... and a run that ends this stage in |amplitude|^2 may build its record
                       // in measured mode (mark_closing_free_groups; a property of the plan, read by the host only)
  uint32_t tbl;        // index into qmle_plan::tbl2 (one uint32 per thread of the workgroup)
  uint32_t tbl_out;    // relayout: scatter table
  uint32_t off[16];
  uint32_t off_out[16];
  uint32_t prod_off;   // product form: float offset of the group's record in the matrix row (behind qmle_plan::mat_floats_unit)
  uint32_t pad[3];
};
static_assert(sizeof(Group2) == 160, "Group2 layout");
constexpr uint8_t kGroupProduct = 2, kGroupProductLow1 = 4, kGroupClosingFree = 8;

enum StageKind : int { ST_DIRECT = 0, ST_TILE = 1, ST_DIAG_ALL = 2 };

struct Stage {
  int kind = ST_TILE;
  int op_begin = 0, op_end = 0;  // range in Plan::dev_ops
  int grp_begin = 0, grp_end = 0;  // range in Plan::op_groups (tile stages)
  int T = 0, L = 0;              // tile qubits, contiguous low bits
  int shift = 0;                 // > 0: the tile is the contiguous run of positions [shift, shift + T) (L = T; the
                                 // first stage of a top-first schedule: one tile per state, stored amplitude by amplitude)
  int n_tile_ops = 0;
  int8_t tile_bits[QMLE_MAX_QUBITS];   // ascending global positions of local bits
  int8_t outer_bits[QMLE_MAX_QUBITS];  // ascending global positions of the rest
  std::vector<int> src_ops;            // reference tape indices covered
  double algo_bytes_per_state = 0;     // SURVEY 8-d bytes of the covered gates
  // Known-zero tracking for runs that start from |0..0> (simulation.py:100): `zero_in` = bit
  // positions p such that every amplitude with bit p set is exactly zero when the stage
  // starts; `touched` = positions the stage's gates mix (non-diagonal targets), which leave
  // the set.  A tile stage never reads such amplitudes, and -- when the next stage is a tile
  // stage too (`next_tile`), which will not read them either -- never launches the tiles that
  // hold nothing else.
  uint32_t zero_in = 0, touched = 0;
  bool next_tile = false;
  // Every gate group sits on 4 bit positions of its own that are all known-zero on input: the
  // output tile is in[live bits] x prod_g (U_g e_0)[group bits] -- k_tile_product writes it
  // from the groups' first columns without staging amplitudes or running gates per tile.
  bool product_ok = false;
  // fast tile path: every gate is a (<= 1 control) 2x2 and T is in k_tile2's range
  bool fast_ok = false;
  int fast_begin = 0, fast_end = 0;  // range in qmle_plan::groups2
  uint32_t fast_gtab = 0;            // index into qmle_plan::tbl2: per-thread global byte offset of
                                     // the lane's first float4 inside the tile (k_tile2 prologue)
  // <Z> of every tile position straight from the registers of the LAST Group2 (k_tile2's multi-tile measuring walk
  // skips that group's scatter and the identity re-layout): behind the group and the X / CX peeled off it, amplitude
  // c (0..15) of work item t sits at logical tile index f = M (e(t, c)) ^ m0, so bit j of f is a parity over bits of
  // c and t plus a constant.  zreg[j] = c mask | t mask << 4 | constant << 15 (zreg_record below); the low six bits
  // of the t mask are lane bits, the rest wave-index bits.  zreg_ok: the records are there (fast_ok, T < n; the last
  // group may be the empty one that only moves the data).
  bool zreg_ok = false;
  uint16_t zreg[16] = {};
  // report only (describe_plan): the group's positions (in-thread bit i), the positions of its thread bits and the
  // X / CX behind it as (control or -1, target) pairs in tile-local positions -- what the records were derived from
  int8_t zreg_bits[4] = {}, zreg_thread_bits[12] = {};
  std::vector<int8_t> zreg_after;
  // Wave-private phases of the measuring walk (k_tile2's register-measuring instantiations).  A phase --
  // staging the loaded tile, a group's gather / gates / in-place scatter -- partitions the tile's 2^T slots among the
  // workgroup's waves; a barrier between two consecutive phases is needed exactly when their partitions differ
  // (Group2::sync bit 0: in front of that group's gather; sync_tile_end: between the last group's gather and the next
  // tile's staging).  slab_load: the tile is loaded and staged so that wave w owns the 2^10 slots whose top T - 10
  // bits are w (lane bits at local bits 1..6, the lane's 8 float4 at 7..9), which is the partition of a first group
  // that leaves the top positions to the wave index; fast_gtab_slab: its per-thread global offsets.  wave_private:
  // no barrier is left in the tile loop.  Computed on the tables as emitted (mark_wave_private_phases), for stages
  // that qualify for the register measurement; every other stage keeps all its barriers.
  struct FastGroupInfo {   // report only: what a group's tables were emitted from (describe_plan)
    uint8_t bits[4];       // the group's positions (in-thread bit i)
    int8_t thread_bits[12];  // position of thread-index bit k
    uint32_t cols[16], cnst; // layout map at that point: logical index e -> slot XOR_{j in e} cols[j] ^ cnst (before sw())
  };
  std::vector<FastGroupInfo> fast_info;  // one per Group2 of [fast_begin, fast_end)
  bool slab_load = false, sync_tile_end = true, wave_private = false;
  uint32_t fast_gtab_slab = 0;
  // Staging by LDS DMA: a wave whose slab nobody else touches between its last gather of one tile and its
  // first gather of the next (slab_load, no barrier in front of the first group, none at the tile's end) lets
  // global_load_lds write the next tile's eight 1 KiB pieces straight into the slab.  Piece u of wave w lands
  // lane-linear at slots u << 7 | w << 10 .. + 127, so lane l fetches the pair whose SWIZZLED index is that slot:
  // local index sw(2 l | u << 7 | w << 10) = sw(2 l | w << 10) ^ u << 7 ^ (u & 3) << 3.  fast_gtab_dma: the global
  // byte offset of sw(2 l | w << 10) per work item; dma_delta[k]: that of local index k << 3 (XORed in per piece).
  // dma_tables: what the tables allow; a run also needs an input without known zeros inside the tile.
  bool dma_tables = false;
  uint32_t fast_gtab_dma = 0, dma_delta[4] = {};
  // The last group through lane swaps: a wave-private DMA walk of >= 2 groups whose last group holds only
  // uncontrolled 1-qubit ops on the positions that are lane bits 4 and 5 of the group in front of it, at in-thread
  // indices 2 and 3, one each (so ops2's codes serve both forms).  The kernel then runs both groups on one gather: behind the
  // first it trades in-thread bit 2 for lane bit 4 and in-thread bit 3 for lane bit 5 (v_permlane16_swap /
  // v_permlane32_swap) and applies the last group's ops where the amplitudes are; the X / CX that the table form puts
  // into the layout between the two groups share no bit with those ops and move behind them, into the records.
  // lane_swap_cross: the targets sit the other way round -- in-thread index 3 on lane bit 4 (the 23-qubit layer's one
  // op), index 2 on lane bit 5 -- and the swaps pair up accordingly.
  // zreg_swap: Stage::zreg for the frame a work item holds then -- in-thread bit i at position zreg_swap_bits[i],
  // thread bit k at zreg_swap_thread_bits[k].  The table form's tables and records stay: known-zero walks take them.
  bool lane_swap_last = false, lane_swap_cross = false;
  uint16_t zreg_swap[16] = {};
  int8_t zreg_swap_bits[4] = {}, zreg_swap_thread_bits[12] = {};
  std::vector<int8_t> zreg_between;  // report only: the X / CX between the last two groups, as zreg_after's pairs
  // report only (describe_plan): indices into the stage's ops2 stream of the ops that run in unit-pivot form and of
  // the carriers that take their chains' pivots (assign_unit_forms)
  std::vector<int> unit_form_ops, scale_carriers;
};
// A stage's lane offsets as runs: local bits 0 .. top -> global positions, contiguous stretches (off, mask, pos).
// Returns their number, or -1 when there are more than four (k_tile2 then reads the offsets from its table).
int stage_lane_runs(const Stage &st, int top, uint32_t off[4], uint32_t mask[4], uint32_t pos[4]);
// the parts of a Stage::zreg record
struct ZregRecord {
  uint32_t wht;   // in-thread bits: index into the 16-point Walsh-Hadamard transform of the squares
  uint32_t lane;  // lane bits
  uint32_t wave;  // wave-index bits
  uint32_t neg;   // 1: the sum enters with a minus sign
};
static inline ZregRecord zreg_record(uint16_t r) {
  return {(uint32_t)r & 15u, ((uint32_t)r >> 4) & 63u, ((uint32_t)r >> 10) & 31u, (uint32_t)r >> 15};
}

struct StageProfile {  // optional HIP-event timing of every stage launch (bench.py)
  bool on = false;
  std::vector<void *> start, stop;  // hipEvent_t pairs
  std::vector<int> stage;           // stage index per recorded pair
  size_t used = 0;
};

struct DevicePlan {  // lazily created by the first run on a device
  int device = -1;     // HIP device the image lives on; runs on another device are refused
  void *blob = nullptr;
  size_t blob_bytes = 0;
  LoweredOp *d_ops = nullptr;
  OpGroup *d_op_groups = nullptr;
  BuildOp *d_build = nullptr;
  BuildGroup *d_groups = nullptr;
  float *d_consts = nullptr;
  LoweredOp *d_ops2 = nullptr;   // fast tile path
  Group2 *d_groups2 = nullptr;
  uint32_t *d_tbl2 = nullptr;
};

// How a batch run ordered its chunks (ChunkPipeline, qmle_engine.hip; LastRun::chunk_loop)
enum { kChunkLoopNone = 0, kChunkLoopOneStream, kChunkLoopStaged, kChunkLoopFree, kChunkLoopAlone };
constexpr const char *kChunkLoopNames[] = {"none", "one_stream", "staged", "free", "alone"};

// How a fused Meyer-Wallach call finished (mw_fused_finish, qmle_mw.hip; LastRun::mw_finish)
enum MwFinish { kMwFinishNone = 0, kMwFinishWholeState, kMwFinishColumns, kMwFinishPerPosition };
constexpr const char *kMwFinishNames[] = {"", "whole-state", "columns", "per-position"};

// What the plan's last run did (describe_plan's *_last_run keys).  Report only: the engine writes it from
// the routes launch_tile returns (TileRoute, qmle_host.h) and never reads it.  run_batch_masks resets all of it first.
struct LastRun {
  // bytes per state that stage 0 of the last batch run really wrote -- its fills and tile-0 stores over its states --
  // when that run left out fills of chunks whose workspace slot already held the zeros; 0 (also after a run that
  // failed): the fresh-buffer figure applies
  uint64_t stage0_written = 0;
  // the last stage's fused <Z> pass in the last batch run: tiles per workgroup (0: no such pass ran), whether it took
  // <Z> from the last group's registers (Stage::zreg), ... in a tile loop without a workgroup barrier
  // (Stage::wave_private), ... staged its tiles by LDS DMA (Stage::dma_tables), ... and ran its last group through lane
  // swaps (Stage::lane_swap_last)
  int measure_tpw = 0;
  bool measure_regs = false, wave_private = false, staging_dma = false, lane_swap = false;
  bool walk_kernel = false;  // ... by k_measure_walk, the straight-line kernel of all-product-form stages (TileRoute::walk_kernel)
  // how the last batch run ordered its chunks (ChunkPipeline::form; a run with one chunk, or with the whole state in
  // the LDS, is a one-stream run)
  int chunk_loop = kChunkLoopNone;
  // bit s: the last launch of tile stage s (batch run or in place; stages 0..63) ran its product-form groups -- every
  // k_tile2 launch does; k_tile and the other readers of dev_ops apply the plain records
  uint64_t product_form_stages = 0;
  // the last batch run's matrix builder formed its angles from the affine map (qmle_run_batch_map from 64 samples on:
  // k_build_matrices_map / k_build_matrices_product_map); false: it read the angle table
  bool matrices_from_map = false;
  // the last batch run's builder wrote measured-mode records (no closing diagonals) for the closing-free
  // groups of its last stage, and that stage's launch ran its product-form groups
  bool measured_form = false;
  // the finish of the last batch run's fused Meyer-Wallach calls (run_mw_fused reports it); kMwFinishNone: that run
  // made no such call
  int mw_finish = kMwFinishNone;
};

}  // namespace qmle

struct qmle_plan {
  int n = 0, n_slots = 0;
  unsigned flags = 0;
  std::vector<qmle_op> ops;
  std::vector<float> consts;
  std::vector<qmle::LoweredOp> lowered;   // after 1-q merging, global positions
  std::vector<std::vector<int>> lowered_src;  // reference ops per lowered op
  std::vector<qmle::LoweredOp> dev_ops;   // per stage, stage-local positions
  std::vector<int> dev_src;               // source op of every dev_op (-1 if merged from several)
  std::vector<qmle::OpGroup> op_groups;   // register-tile groups of the tile stages
  std::vector<qmle::LoweredOp> ops2;      // fast tile path: ops of the Group2 groups
  std::vector<uint8_t> ops2_perm_tail;    // ... per op: only X / CX follow on its wire and on the wires they spread it to
                                          // (the stage's op order; build_fast_groups, for mark_closing_free_groups)
  std::vector<qmle::Group2> groups2;
  std::vector<uint32_t> tbl2;             // per-thread LDS byte addresses of the Group2 groups
  std::vector<qmle::BuildOp> build_ops;
  std::vector<qmle::BuildGroup> groups;   // needed-first: [0, n_groups_needed) are read by the forward tile / direct kernels
  int n_groups_needed = 0;
  int n_product_groups = 0;               // ... the last of which build product-form records (kBuildProduct; a kernel of their own)
  std::vector<qmle::Stage> stages;
  uint32_t mat_floats = 0;                // per-sample matrix row length (the stride of the rows)
  uint32_t mat_floats_unit = 0;           // ... end of the unit-form records (describe_plan's "mat_floats"); the product-form
                                          // records of Group2 groups follow (assign_product_forms)
  uint32_t mat_floats_old = 0;            // ... of which the plain records, one per lowered operator (a function of the
                                          // tape and the flags alone); the unit-form records of ops2 follow
  int fold_groups = 0;                    // most gate groups of any Stage::product_ok stage
  double model_cost = 0.0;                // pass-cost model of the chosen schedule (us per state at n = 24 scale)
  int chosen_candidate = -1;              // number of the schedule candidate the model picked (choose_schedule, candidate_of)
  // plan autotuner (qmle_plan_autotune): a forced candidate / last-stage padding for this compile (-1: the
  // cost model resp. the QMLE_FORCE_CAND / QMLE_PAD_HIGH tuning switches), and every allowed candidate with
  // its model cost, cheapest first
  int force_candidate = -1, pad_high = -1;
  std::vector<std::pair<double, int>> cand_ranking;
  bool autotuned = false;
  uint64_t schedule_serial = 0;           // times qmle_plan_autotune gave this plan another schedule (adopt_schedule)
  // The same tape compiled for runs from |0..0> only (qmle_run_batch): its first stage may stage a
  // wider tile (it computes one tile per state whatever the size).  Owned; used by run_batch_masks
  // in place of this plan; qmle_apply_inplace / the adjoint sweep keep using this plan's stages.
  qmle_plan *zero_variant = nullptr;
  // complex128 engine (qmle_run_batch_f64): device copy of `lowered` + the constant blob as doubles
  // (lazily created); `consts64` optionally holds the caller's constants at full precision
  void *f64_blob = nullptr;
  int f64_device = -1;
  size_t n_user_consts = 0;               // constants handed to qmle_plan_create (the blob grows by permuted copies)
  std::vector<double> consts64;
  bool whole_state_lds = false;
  int tile_T = 0, tile_L = 0;
  double algo_bytes_per_state = 0;
  qmle::LastRun last_run;                 // report only (describe_plan)
  qmle::DevicePlan dev;
  qmle::StageProfile prof;
  // <Z> measurements only: trailing gates that map basis states to basis states (CX, SWAP)
  // or only add phases (diagonal gates) never touch a statevector -- they are folded into
  // the observables (Z_t -> Z_c Z_t under CX[c,t]) and `expval_child` runs the rest.
  qmle_plan *expval_child = nullptr;
  std::vector<qmle_op> absorbed;        // the folded gates, tape order
  double absorbed_algo_bytes = 0;       // their SURVEY 8-d bytes (credited to the last stage)
  double extra_algo_last_stage = 0;     // child side of the same number
  // adjoint sweep in LDS: device copies of the reverse tape (global positions) and its generator
  // terms, uploaded once per (plan, terms) -- owned by the REVERSE plan
  void *adj_blob = nullptr;
  uint64_t adj_hash = 0;
  // fused adjoint tile passes: per dev_op derivative index / generator type, per stage term
  // -> (gradient column, coefficient) tables
  void *adjf_blob = nullptr;
  uint64_t adjf_hash = 0;
};

// internal plan flag (bit 25; not part of the ABI): the plan is executed by qmle_run_batch only
#define QMLE_PLAN_INTERNAL_ZERO_RUN (1u << 25)

namespace qmle {
int compile_plan(qmle_plan *p);  // qmle_plan.cpp: validate_tape, lower_tape, reorder_low_bits_first, choose_schedule, ...
// Split `ops` into the gates a <Z> measurement needs (`kept`) and the absorbable tail.
void split_expval_tail(const std::vector<qmle_op> &ops, int n, std::vector<qmle_op> &kept,
                       std::vector<qmle_op> &absorbed);
// Z on `wire` pulled back through the absorbed gates: bit w set <=> Z_w in the parity.
uint32_t pull_back_z(const std::vector<qmle_op> &absorbed, int wire);
std::string describe_plan(const qmle_plan *p);
// Which kernel runs a tile stage.  The first four are what expval_kernel_of answers (and index describe_plan's names).
enum TileFamily : int {
  TF_TILE = 0,              // k_tile<DENSE4, MW>
  TF_REG_MEASURE = 1,       // k_reg_measure<false>
  TF_REG_MEASURE_FOLD = 2,  // k_reg_measure<true>: gates folded into columns
  TF_REG_MEASURE_MONO = 3,  // k_reg_measure_mono<Q, PAIR, NT>
  TF_TILE2 = 4,             // k_tile2<NT, MEASURE, MULTI, WS, MW, MASKS>
  TF_TILE_PRODUCT = 5,      // k_tile_product
  TF_PRODUCT_STREAM = 6,    // k_product_stream<NT>
};
constexpr const char *kTileFamilyNames[] = {"k_tile",  "k_reg_measure",  "k_reg_measure_fold", "k_reg_measure_mono",
                                            "k_tile2", "k_tile_product", "k_product_stream"};
inline bool is_reg_measure(TileFamily f) { return f >= TF_REG_MEASURE && f <= TF_REG_MEASURE_MONO; }
// Which kernel measures <Z> / Z parities out of stage `si` when it is the last one of a run from |0..0>: TF_TILE (the
// tile kernels' epilogues) or one of k_reg_measure*.  `sparse`: known-zero tracking is on for the run.
TileFamily expval_kernel_of(const qmle_plan *p, size_t si, bool sparse);
// Stage `si` QUALIFIES for <Z> from the last group's registers (Stage::zreg): it is the last of several, has a k_tile2
// description with records (any last Group2 will do, the empty data-moving one included) and no known-zero TILES on
// input -- known zeros INSIDE the tile are fine, idle work items hand over zeros.  Whether a run takes that path is
// decided per launch: only a multi-tile TM_EXPVAL_PARTIAL walk does (launch_tile); a run that hands the stage to
// k_reg_measure*, measures folded-CX parities (TM_EXPVAL_MASKS) or has too few tiles for a walk does not, and
// LastRun::measure_regs says which it was.
bool qualifies_for_register_measure(const qmle_plan *p, size_t si);
// Stage::zero_in as a tile pass sees it: *local = tile-local bits, *outer = tile-index bits that are known zero
void stage_known_zeros(const qmle_plan *p, const Stage &st, uint32_t *local, uint32_t *outer);
// ... and its walk stages by LDS DMA whenever it runs: Stage::dma_tables, and no known zeros inside the tile
// (walk_by_dma: the same with the known-zero local bits of the launch in hand).
bool walk_by_dma(const Stage &st, uint32_t zin_local);
bool stages_by_dma(const qmle_plan *p, size_t si);
// ... and its last group runs through lane swaps then (Stage::lane_swap_last rides on the DMA form)
inline bool walk_by_lane_swap(const Stage &st, bool by_dma) { return st.fast_ok && st.lane_swap_last && by_dma; }
double algo_bytes(const qmle_op &op, int n);
constexpr int kFastMinT = 10, kFastMaxT = 13;  // k_tile2: 2^(T-4) threads, 8 float4 per thread
constexpr int kLdsMaxQubits = 14;       // 2^14 * 8 B = 128 KiB <= 160 KiB LDS/CU
constexpr int kDefaultTileBits = 13;    // 64 KiB tile -> 2 workgroups per CU
constexpr int kDefaultLowBits = 7;      // 128 amplitudes = 1 KiB contiguous per wave load
}  // namespace qmle
