// Host-side plan compiler: tape validation, lowering to controlled-2x2 / 4x4
// primitives, commutation-aware merging of 1-qubit gates, and greedy scheduling
// of the lowered ops into HBM passes ("stages").  No HIP calls in this file, so
// plans can be built and inspected on a machine without a GPU.
//
// What is being replaced: jax traces the circuit once and XLA emits one
// out-of-place einsum per gate (qml_essentials/simulation.py:91-104).  Here the
// tape is compiled into a few passes; each pass stages a 2^T-amplitude tile in
// LDS and applies every gate whose wires fall inside the tile.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <functional>
#include <sstream>

#include "qmle_internal.h"

namespace qmle {

namespace {

struct OpInfo {
  int n_wires;
  int n_params;
  bool has_const;
};

bool op_info(int opcode, OpInfo *info) {
  switch (opcode) {
    case QMLE_OP_ID: case QMLE_OP_X: case QMLE_OP_Y: case QMLE_OP_Z:
    case QMLE_OP_H: case QMLE_OP_S:
      *info = {1, 0, false}; return true;
    case QMLE_OP_RX: case QMLE_OP_RY: case QMLE_OP_RZ:
      *info = {1, 1, false}; return true;
    case QMLE_OP_ROT:
      *info = {1, 3, false}; return true;
    case QMLE_OP_CX: case QMLE_OP_CY: case QMLE_OP_CZ: case QMLE_OP_SWAP:
      *info = {2, 0, false}; return true;
    case QMLE_OP_CRX: case QMLE_OP_CRY: case QMLE_OP_CRZ: case QMLE_OP_CPHASE:
    case QMLE_OP_RXX: case QMLE_OP_RYY: case QMLE_OP_RZZ: case QMLE_OP_RZX:
      *info = {2, 1, false}; return true;
    case QMLE_OP_CCX: case QMLE_OP_CSWAP:
      *info = {3, 0, false}; return true;
    case QMLE_OP_MAT1:
      *info = {1, 0, true}; return true;
    case QMLE_OP_MAT2:
      *info = {2, 0, true}; return true;
    case QMLE_OP_MAT1_ROW:  // (slot[0]: the first of 8 / 32 columns -- validate_tape checks where they end)
      *info = {1, 1, false}; return true;
    case QMLE_OP_MAT2_ROW:
      *info = {2, 1, false}; return true;
    case QMLE_OP_DIAG_ALL:
      *info = {-1, 1, true}; return true;
    case QMLE_OP_MAT4:
      *info = {4, 0, true}; return true;
    default:
      return false;
  }
}

bool is_diag_opcode(int opcode) {
  switch (opcode) {
    case QMLE_OP_ID: case QMLE_OP_Z: case QMLE_OP_S: case QMLE_OP_RZ:
    case QMLE_OP_CZ: case QMLE_OP_CRZ: case QMLE_OP_CPHASE: case QMLE_OP_RZZ:
      return true;
    default:
      return false;
  }
}

inline uint64_t bit(int p) { return 1ull << p; }

uint64_t op_mask(const LoweredOp &o, int n) {
  if (o.kind == LK_DIAG_ALL) return n >= 64 ? ~0ull : (bit(n) - 1);
  uint64_t m = bit(o.t0);
  if (o.t1 >= 0) m |= bit(o.t1);
  if (o.c0 >= 0) m |= bit(o.c0);
  if (o.c1 >= 0) m |= bit(o.c1);
  return m;
}

// the positions outside a stage's tile, as a mask
uint32_t outer_mask(const Stage &st, int n) {
  uint32_t m = 0;
  for (int i = 0; i < n - st.T; ++i) m |= 1u << st.outer_bits[i];
  return m;
}

// bit j of the result = bit pos[j] of v, for j < count
uint32_t gather_bits(uint32_t v, const int8_t *pos, int count) {
  uint32_t out = 0;
  for (int j = 0; j < count; ++j)
    if (v & (1u << pos[j])) out |= 1u << j;
  return out;
}

// the gate of the tape that lowered operator i stands for, -1 when it is a product of several
int single_src(const qmle_plan *p, size_t i) { return p->lowered_src[i].size() == 1 ? p->lowered_src[i][0] : -1; }

}  // namespace

// SURVEY.md 8-d / BASELINE.md section 3: algorithmic bytes per state of one
// reference gate (complex64, D = 2^n).
double algo_bytes(const qmle_op &op, int n) {
  const double D = (double)(1ull << n);
  switch (op.opcode) {
    case QMLE_OP_ID: return 0.0;
    case QMLE_OP_CX: case QMLE_OP_CY: case QMLE_OP_CRX: case QMLE_OP_CRY:
    case QMLE_OP_CRZ: return 8.0 * D;
    case QMLE_OP_CZ: case QMLE_OP_CPHASE: case QMLE_OP_CCX: case QMLE_OP_CSWAP:
      return 4.0 * D;
    default: return 16.0 * D;
  }
}

// Partition the ops of one tile stage into register-tile groups (<= 4 tile-local bits
// per group, dependency order preserved: an op may only move ahead of ops it shares no
// bit with).  Rewrites dev_ops[st.op_begin, st.op_end) into group order.
static void group_stage_ops(qmle_plan *p, Stage &st) {
  const int nops = st.op_end - st.op_begin;
  st.grp_begin = (int)p->op_groups.size();
  std::vector<LoweredOp> src(p->dev_ops.begin() + st.op_begin, p->dev_ops.begin() + st.op_end);
  std::vector<int> src_id(p->dev_src.begin() + st.op_begin, p->dev_src.begin() + st.op_end);
  std::vector<LoweredOp> out;
  std::vector<int> out_id;
  out.reserve(nops);
  std::vector<char> done(nops, 0);
  const bool regs_ok = st.T >= 4 && !(p->flags & QMLE_PLAN_NO_REGTILE);
  // (round 5: an uncontrolled dense 4x4 joins a register-tile run as well -- the noisy model's superoperators sit
  // between every pair of gates and cost an LDS sweep each otherwise.  Plans that keep every gate its own operator
  // (QMLE_PLAN_NO_MERGE: the adjoint sweep's, whose tile kernel knows GK_REG4 only) do not)
  const bool reg2q = regs_ok && !(p->flags & QMLE_PLAN_NO_MERGE);
  auto groupable = [&](const LoweredOp &o) {
    return regs_ok && ((o.kind == LK_1Q && o.nc <= 1) || (reg2q && o.kind == LK_2Q && o.nc == 0));
  };
  auto mask_of = [&](const LoweredOp &o) -> uint32_t {
    if (o.kind == LK_DIAG_ALL) return st.T >= 32 ? ~0u : ((1u << st.T) - 1u);
    uint32_t m = 1u << o.t0;
    if (o.t1 >= 0) m |= 1u << o.t1;
    if (o.c0 >= 0) m |= 1u << o.c0;
    if (o.c1 >= 0) m |= 1u << o.c1;
    return m;
  };
  int n_done = 0;
  while (n_done < nops) {
    int first = 0;
    while (done[first]) ++first;
    OpGroup g{};
    g.op_begin = (uint32_t)(st.op_begin + out.size());
    if (src[first].kind == LK_4Q && st.T >= 4) {
      // gather order = ascending tile-local bit; permute the 16x16 matrix (given in wire
      // order, first wire = MSB) into that order once, on the host
      LoweredOp o = src[first];
      const int pos4[4] = {o.t0, o.t1, o.c0, o.c1};  // wire order, MSB first
      int sorted[4] = {pos4[0], pos4[1], pos4[2], pos4[3]};
      std::sort(sorted, sorted + 4);
      int rank_of[4];  // matrix bit (3 - j) of wire j  ->  gather bit = rank of its position
      for (int j = 0; j < 4; ++j)
        rank_of[j] = (int)(std::find(sorted, sorted + 4, pos4[j]) - sorted);
      auto to_wire_index = [&](int c) {  // gather index c -> matrix index in wire order
        int m = 0;
        for (int j = 0; j < 4; ++j)
          if (c & (1 << rank_of[j])) m |= 1 << (3 - j);
        return m;
      };
      const size_t src_off = o.mat_off, dst_off = p->consts.size();
      p->consts.resize(dst_off + 512);
      for (int r = 0; r < 16; ++r)
        for (int c = 0; c < 16; ++c) {
          const int mr = to_wire_index(r), mc = to_wire_index(c);
          p->consts[dst_off + 2 * (r * 16 + c)] = p->consts[src_off + 2 * (mr * 16 + mc)];
          p->consts[dst_off + 2 * (r * 16 + c) + 1] = p->consts[src_off + 2 * (mr * 16 + mc) + 1];
        }
      o.mat_off = (uint32_t)dst_off;
      g.kind = GK_DENSE4;
      g.n_ops = 1;
      for (int j = 0; j < 4; ++j) g.bits[j] = (uint8_t)sorted[j];
      out.push_back(o);
      out_id.push_back(src_id[first]);
      done[first] = 1;
      ++n_done;
      p->op_groups.push_back(g);
      continue;
    }
    if (!groupable(src[first])) {
      g.kind = GK_SWEEP;
      g.n_ops = 1;
      out.push_back(src[first]);
      out_id.push_back(src_id[first]);
      done[first] = 1;
      ++n_done;
      p->op_groups.push_back(g);
      continue;
    }
    g.kind = GK_REG4;
    uint32_t G = 0, blocked = 0;
    std::vector<int> mem;
    for (int i = first; i < nops && mem.size() < 255; ++i) {
      if (done[i]) continue;
      const uint32_t m = mask_of(src[i]);
      if ((m & blocked) || !groupable(src[i])) {
        blocked |= m;
      } else if (__builtin_popcount(G | m) <= 4) {
        G |= m;
        mem.push_back(i);
      } else {
        blocked |= m;
      }
    }
    // pad to 4 bits: prefer positions >= 5 (bank-conflict-free gathers), then anything free
    for (int b = 5; b < st.T && __builtin_popcount(G) < 4; ++b) G |= 1u << b;
    for (int b = 0; b < st.T && __builtin_popcount(G) < 4; ++b) G |= 1u << b;
    int8_t local_of[32];
    int k = 0;
    for (int b = 0; b < st.T; ++b) {
      local_of[b] = -1;
      if (G & (1u << b)) { g.bits[k] = (uint8_t)b; local_of[b] = (int8_t)k++; }
    }
    g.n_ops = (uint8_t)mem.size();
    for (int i : mem) {
      LoweredOp o = src[i];
      o.t0 = local_of[(int)o.t0];
      if (o.kind == LK_2Q) {
        o.t1 = local_of[(int)o.t1];
        g.kind = GK_REG4X;
      }
      if (o.c0 >= 0) o.c0 = local_of[(int)o.c0];
      out.push_back(o);
      out_id.push_back(src_id[i]);
      done[i] = 1;
      ++n_done;
    }
    p->op_groups.push_back(g);
  }
  std::copy(out.begin(), out.end(), p->dev_ops.begin() + st.op_begin);
  std::copy(out_id.begin(), out_id.end(), p->dev_src.begin() + st.op_begin);
  st.grp_end = (int)p->op_groups.size();
}

// ---- fast tile path: perm-fused register-tile groups (Group2) --------------------------------
// `src`: the stage's ops in a valid execution order, TILE-local bit positions.  Greedy like
// group_stage_ops, except that X / CX never cost a group of their own:
//   * one that touches no bit of the group being formed (and no blocked bit) is applied to the
//     layout map at once -- the group's gather table already sees it;
//   * one at the END of a group's op list is peeled off and applied to the layout map after the
//     group (its scatter stays in place);
//   * only an X / CX sandwiched between the group's dense gates runs in registers (8 moves).
static inline uint32_t swz(uint32_t e) { return e ^ (((e >> 5) & 15u) << 1); }  // = sw() in qmle_dev.h

static void mark_wave_private_phases(qmle_plan *p, Stage &st, bool measured);

// What qualifies_for_register_measure asks of a stage's place and input, known while the stage is being built: it is
// the last of several, a tile smaller than the state, and no known-zero TILES come in (`zero_in`: Stage::zero_in).
static bool placed_for_register_measure(const qmle_plan *p, const Stage &st, uint32_t zero_in, bool first, bool last) {
  if (first || !last || st.T >= p->n) return false;
  if (p->flags & QMLE_PLAN_NO_SPARSE) return true;
  return !(zero_in & outer_mask(st, p->n));  // known-zero TILES keep one tile per workgroup and its epilogue
}

// The two GF(2)-affine maps of a stage's tile indices that build_fast_groups keeps while it forms the groups:
//   L, the layout map: logical tile index e lives at physical slot L(e) = XOR_{j in e} Lcol[j] ^ Lconst;
//   M: logical index in the frame of the last emitted group -> logical index now, and `since`, the X / CX that make
//   up M, in order: (control or -1, target) pairs (describe_plan).
struct LayoutMaps {
  int T;
  uint32_t Lcol[16], Lconst = 0, Mcol[16], Mconst = 0;
  std::vector<int8_t> since;
  explicit LayoutMaps(int T_) : T(T_) {
    for (int j = 0; j < 16; ++j) Lcol[j] = Mcol[j] = 1u << j;
  }
  void reset_M() {
    for (int j = 0; j < T; ++j) Mcol[j] = 1u << j;
    Mconst = 0;
    since.clear();
  }
  uint32_t L_of(uint32_t e) const {
    uint32_t v = Lconst;
    for (int j = 0; j < T; ++j)
      if (e & (1u << j)) v ^= Lcol[j];
    return v;
  }
  uint32_t M_lin(uint32_t e) const {  // the linear part of M
    uint32_t v = 0;
    for (int j = 0; j < T; ++j)
      if (e & (1u << j)) v ^= Mcol[j];
    return v;
  }
  bool is_identity() const {  // (the layout map)
    if (Lconst) return false;
    for (int j = 0; j < T; ++j)
      if (Lcol[j] != (1u << j)) return false;
    return true;
  }
  void apply_perm(const LoweredOp &o) {  // an X / CX behind everything applied so far
    const int t = o.t0;
    since.push_back(o.nc == 0 ? (int8_t)-1 : o.c0);
    since.push_back(o.t0);
    if (o.nc == 0) {
      Lconst ^= Lcol[t];
      Mconst ^= 1u << t;
    } else {
      const int c = o.c0;
      Lcol[c] ^= Lcol[t];
      for (int j = 0; j < T; ++j) Mcol[j] ^= ((Mcol[j] >> c) & 1u) << t;
      Mconst ^= ((Mconst >> c) & 1u) << t;
    }
  }
};

static void group_positions(uint32_t G, int T, int gb[4]) {  // the four positions of a group, ascending
  int k = 0;
  for (int j = 0; j < T && k < 4; ++j)
    if (G & (1u << j)) gb[k++] = j;
}

// What build_fast_groups keeps while it forms a stage's groups, and what its epilogues read of it.
struct FastGroupBuilder {
  qmle_plan *p;
  Stage &st;
  const std::vector<LoweredOp> &src;
  const bool measured;
  const int T, nops;
  const uint32_t nt;
  LayoutMaps maps;
  // the maps as they stood when the newest group was emitted: its M is the X / CX between that group and the one in
  // front of it (Stage::lane_swap_last)
  LayoutMaps before_last;
  // known-zero tile-local bits along the stage's execution (runs from |0..0>, Stage::zero_in):
  // a gate that is not diagonal takes its target out of the set, controls stay.  A work item
  // whose base index meets the set outside its group's bits holds 16 exact zeros: bit 0 of its
  // table entry says so (the kernel honours it only in runs that track known zeros).
  uint32_t Z;
  int pos_of[16];  // thread index bit k of the newest group's work items -> tile-local position (choose_thread_bits)
  std::vector<char> done;
  int n_done = 0;
  std::vector<int> held;  // X / CX kept back for behind the last group
  int last_group = -1;
  uint32_t last_G = 0;
  const uint32_t slab_bits;

  FastGroupBuilder(qmle_plan *p_, Stage &st_, const std::vector<LoweredOp> &src_, uint32_t zin_local, bool measured_)
      : p(p_), st(st_), src(src_), measured(measured_), T(st_.T), nops((int)src_.size()), nt(1u << (st_.T - 4)),
        maps(st_.T), before_last(st_.T), Z(zin_local), done(src_.size(), 0),
        slab_bits(st_.T > 10 ? ((1u << st_.T) - 1u) & ~1023u : 0u) {}

  static bool is_perm(const LoweredOp &o) { return (o.flags & LF_PERMX) != 0; }
  static uint32_t mask_of(const LoweredOp &o) {
    uint32_t m = 1u << o.t0;
    if (o.c0 >= 0) m |= 1u << o.c0;
    return m;
  }
  void choose_thread_bits(uint32_t G, bool keep_order);
  uint32_t deposit(uint32_t t) const {  // bits of t into the positions outside the newest group's
    uint32_t e = 0;
    for (int k = 0; k < T - 4; ++k) e |= ((t >> k) & 1u) << pos_of[k];
    return e;
  }
  void emit_tables(Group2 &g, uint32_t G);
  // (Correctness rests on the scan alone: an X / CX that no later op touches commutes with everything behind it.  The
  // column test only says when waiting pays: X[t] XORs column t into the constant, CX[c -> t] into column c, so a
  // column t that holds a slab bit is what would move slots between slabs.)
  bool keeps_back(int i) const {
    if (!measured || !(maps.Lcol[(int)src[i].t0] & slab_bits)) return false;
    const uint32_t m = mask_of(src[i]);
    for (int j = i + 1; j < nops; ++j)
      if (!done[j] && (mask_of(src[j]) & m)) return false;
    return true;
  }
  // Rule 1 of mark_closing_free_groups for op i alone (the rule of a group is the AND over its members: the spread
  // of a union of wires is the union of the spreads): in the stage's op order, every op behind i that touches a wire
  // i's result has reached is an X / CX -- which hands it on to its other wire
  bool perm_tail(int i) const {
    uint32_t taint = mask_of(src[i]);
    for (int j = i + 1; j < nops; ++j) {
      const uint32_t m = mask_of(src[j]);
      if (!(m & taint)) continue;
      if (!is_perm(src[j])) return false;
      taint |= m;
    }
    return true;
  }
  void apply_perm(const LoweredOp &o) {
    Z &= ~(1u << o.t0);
    maps.apply_perm(o);
  }
  void to_layout(int i) {  // X / CX number i leaves the op list for the layout map, now or behind the last group
    if (keeps_back(i)) held.push_back(i);
    else apply_perm(src[i]);
    done[i] = 1;
    ++n_done;
  }
  void emit_group(const std::vector<int> &mem, const std::vector<int> &trailing);
  void form_groups();
};

// Thread index bit k of a group's work items -> tile-local position pos_of[k] (outside the group's
// bits).  Any bijection is correct; WHICH one decides the LDS bank conflicts of the group's 32
// accesses: slot(thread, c) = P(thread) ^ Q(c) with P linear over GF(2), so a ds_write_b64's 16-lane
// groups are conflict-free iff thread bits 0..3 land on columns that are independent in slot bits
// 0..3 (16 slots = 32 banks), and a ds_read_b64's 32-lane groups iff bits 0..4 are independent in
// slot bits 0..4 (MI355X_MICROARCH.md, LDS table).  Ascending order -- the round-2 choice -- left
// 33-38 % of the LDS cycles of the whole-state kernels to conflicts (SQ_LDS_BANK_CONFLICT,
// profiles/r04_ws_sq_*.txt).  Only the lane bits are permuted: the wave index keeps the highest
// positions, where the known zeros of a run from |0..0> sit (whole waves of idle work items skip).
void FastGroupBuilder::choose_thread_bits(uint32_t G, bool keep_order) {
  const uint32_t *Lcol = maps.Lcol;
  int freep[16], nf = 0;
  for (int j = 0; j < T; ++j)
    if (!(G & (1u << j))) freep[nf++] = j;
  for (int k = 0; k < nf; ++k) pos_of[k] = freep[k];
  const int lanes = nf < 6 ? nf : 6;
  if (keep_order || lanes < 2) return;
  uint32_t basis[8];
  int nb = 0;
  auto independent = [&](uint32_t v) {  // reduce v by the basis; keep it when something is left
    for (int i = 0; i < nb; ++i)
      if ((v ^ basis[i]) < v) v ^= basis[i];
    if (!v) return false;
    basis[nb++] = v;
    for (int i = nb - 1; i > 0 && basis[i] > basis[i - 1]; --i) std::swap(basis[i], basis[i - 1]);
    return true;
  };
  bool used[16] = {};
  int order[16], no = 0;
  for (int k = 0; k < lanes && no < 4; ++k)  // four columns independent in slot bits 0..3
    if (independent(swz(Lcol[freep[k]]) & 0xFu)) { order[no++] = k; used[k] = true; }
  nb = 0;
  for (int i = 0; i < no; ++i) (void)independent(swz(Lcol[freep[order[i]]]) & 0x1Fu);
  const int first4 = no;
  for (int k = 0; k < lanes && no < first4 + 1; ++k)  // a fifth, independent in slot bits 0..4
    if (!used[k] && independent(swz(Lcol[freep[k]]) & 0x1Fu)) { order[no++] = k; used[k] = true; }
  // fewer than four independent columns exist: the group's own bits own those banks -- fill up
  // (thread bits 4 / 5 only choose the lane group of a write, bit 5 that of a read)
  for (int k = 0; k < lanes; ++k)
    if (!used[k]) order[no++] = k;
  for (int k = 0; k < lanes; ++k) pos_of[k] = freep[order[k]];
}

void FastGroupBuilder::emit_tables(Group2 &g, uint32_t G) {
  int gb[4];
  group_positions(G, T, gb);
  // (the idle-work-item flags below are only read by tiled runs that track known zeros)
  choose_thread_bits(G, (Z & ~G) != 0 && T < p->n && !(p->flags & QMLE_PLAN_NO_SPARSE));
  g.sync = 1;
  Stage::FastGroupInfo info{};
  for (int j = 0; j < 4; ++j) info.bits[j] = (uint8_t)gb[j];
  for (int t = 0; t < T - 4; ++t) info.thread_bits[t] = (int8_t)pos_of[t];
  for (int j = 0; j < T; ++j) info.cols[j] = maps.Lcol[j];
  info.cnst = maps.Lconst;
  st.fast_info.push_back(info);
  g.tbl = (uint32_t)p->tbl2.size();
  for (uint32_t t = 0; t < nt; ++t) {
    const uint32_t e = deposit(t);
    p->tbl2.push_back((swz(maps.L_of(e)) << 3) | ((e & Z & ~G) ? 1u : 0u));
  }
  for (int c = 0; c < 16; ++c) {
    uint32_t v = 0;
    for (int j = 0; j < 4; ++j)
      if (c & (1 << j)) v ^= maps.Lcol[gb[j]];
    g.off[c] = swz(v) << 3;
  }
}

// One group: its tables, its members `mem` with group-local bits and their dispatch codes, then the X / CX `trailing`
// behind it.
void FastGroupBuilder::emit_group(const std::vector<int> &mem, const std::vector<int> &trailing) {
  uint32_t G = 0;
  for (int i : mem) G |= mask_of(src[i]);
  for (int b = 5; b < T && __builtin_popcount(G) < 4; ++b) G |= 1u << b;
  for (int b = 0; b < T && __builtin_popcount(G) < 4; ++b) G |= 1u << b;
  int8_t local_of[16];
  for (int b = 0, k = 0; b < T; ++b) local_of[b] = (G & (1u << b)) ? (int8_t)k++ : (int8_t)-1;
  Group2 g;
  std::memset(&g, 0, sizeof(g));
  g.op_begin = (uint32_t)p->ops2.size();
  g.n_ops = (uint16_t)mem.size();
  emit_tables(g, G);
  for (int i : mem)
    if (!(src[i].flags & LF_DIAG)) Z &= ~(1u << src[i].t0);
  for (int i : mem) {
    LoweredOp o = src[i];
    o.t0 = local_of[(int)o.t0];
    if (o.c0 >= 0) o.c0 = local_of[(int)o.c0];
    const int base = is_perm(o) ? (o.nc ? FC_CX : FC_X)
                     : (o.flags & LF_DIAG) ? (o.nc ? FC_CDIAG : FC_DIAG)
                                           : (o.nc ? FC_CDENSE : FC_DENSE);
    o.pad = (uint8_t)(base + (o.nc ? 3 * o.c0 + (o.t0 - (o.t0 > o.c0 ? 1 : 0)) : o.t0));
    p->ops2.push_back(o);
    p->ops2_perm_tail.push_back(perm_tail(i) ? 1 : 0);
    done[i] = 1;
    ++n_done;
  }
  before_last = maps;
  maps.reset_M();
  for (int i : trailing) to_layout(i);
  last_group = (int)p->groups2.size();
  last_G = G;
  p->groups2.push_back(g);
}

void FastGroupBuilder::form_groups() {
  while (n_done < nops) {
    uint32_t G = 0, touched = 0, blocked = 0;
    std::vector<int> mem, after;  // `after`: X / CX applied to the layout behind the group
    for (int i = 0; i < nops; ++i) {
      if (done[i]) continue;
      const uint32_t m = mask_of(src[i]);
      if (m & blocked) { blocked |= m; continue; }
      if (is_perm(src[i])) {
        if (!(m & touched)) {  // independent of the group: layout only, before the group
          to_layout(i);
        } else if ((m & ~G) == 0 && mem.size() < 4000) {
          mem.push_back(i);  // inside the group's bits: stays in registers unless peeled below
        } else {             // would cost the group a bit position: behind the group instead
          after.push_back(i);
          blocked |= m;
        }
        continue;
      }
      if (__builtin_popcount(G | m) <= 4 && mem.size() < 4000) {
        G |= m;
        touched |= m;
        mem.push_back(i);
      } else {
        blocked |= m;
      }
    }
    if (mem.empty()) continue;  // only layout changes were left (`after` needs a member: empty too)
    // an X / CX that commutes with every later member of the group leaves it for the layout
    uint32_t later = 0;
    std::vector<int> keep;
    for (size_t k = mem.size(); k-- > 0;) {
      const int i = mem[k];
      const uint32_t m = mask_of(src[i]);
      if (is_perm(src[i]) && !(m & later)) {
        after.push_back(i);
      } else {
        later |= m;
        keep.insert(keep.begin(), i);
      }
    }
    std::sort(after.begin(), after.end());
    emit_group(keep, after);
  }
  if (last_group < 0) {  // nothing but layout changes (or no gate at all): an empty group moves the data
    Group2 g;
    std::memset(&g, 0, sizeof(g));
    g.op_begin = (uint32_t)p->ops2.size();
    last_G = 0xFu << (T >= 9 ? 5 : 0);
    emit_tables(g, last_G);
    maps.reset_M();
    last_group = (int)p->groups2.size();
    p->groups2.push_back(g);
  }
  for (int i : held) apply_perm(src[i]);  // (they commute with every op behind them: tape order among themselves)
}

// The epilogue (store / measure) reads the tile in the identity layout: the last group scatters through a table of its
// own.  A thread holds logical index e of the group's frame; its final logical index is M(e).
static void emit_relayout(const FastGroupBuilder &b) {
  if (b.maps.is_identity()) return;
  qmle_plan *p = b.p;
  Group2 &g = p->groups2[b.last_group];
  int gb[4];
  group_positions(b.last_G, b.T, gb);
  g.relayout = 1;
  g.tbl_out = (uint32_t)p->tbl2.size();
  for (uint32_t t = 0; t < b.nt; ++t) p->tbl2.push_back(swz(b.maps.M_lin(b.deposit(t)) ^ b.maps.Mconst) << 3);
  for (int c = 0; c < 16; ++c) {
    uint32_t e = 0;
    for (int j = 0; j < 4; ++j)
      if (c & (1 << j)) e |= 1u << gb[j];
    g.off_out[c] = swz(b.maps.M_lin(e)) << 3;
  }
}

// <Z> from the last group's registers (Stage::zreg): amplitude c of work item t holds index e(t, c) of the group's
// frame (thread bit k at position pos_of[k], in-thread bit i at the group's i-th position) and ends at logical
// index M e ^ Mconst; bit j of that is the parity of e under row j of M, plus bit j of Mconst
static void emit_zreg_records(const FastGroupBuilder &b, Stage &st) {
  const int T = b.T;
  const LayoutMaps &m = b.maps;
  st.zreg_ok = false;
  std::memset(st.zreg, 0, sizeof(st.zreg));
  if (T >= b.p->n) return;  // (last_group: a gate group, or the empty one that only moves the data)
  int gb[4];
  group_positions(b.last_G, T, gb);
  for (int j = 0; j < T; ++j) {
    uint32_t rec = ((m.Mconst >> j) & 1u) << 15;
    for (int i = 0; i < 4; ++i) rec |= ((m.Mcol[gb[i]] >> j) & 1u) << i;
    for (int t = 0; t < T - 4; ++t) rec |= ((m.Mcol[b.pos_of[t]] >> j) & 1u) << (4 + t);
    st.zreg[j] = (uint16_t)rec;
  }
  for (int i = 0; i < 4; ++i) st.zreg_bits[i] = (int8_t)gb[i];
  for (int t = 0; t < T - 4; ++t) st.zreg_thread_bits[t] = (int8_t)b.pos_of[t];
  st.zreg_ok = true;
}

// The last group through lane swaps (Stage::lane_swap_last).  Behind the ops of the group in front of it, work item t
// holds amplitude c at index e(t, c) of THAT group's frame.  The X / CX between the two groups (N) touch none of
// the last group's positions, so its ops commute to the front of them: they run in that frame, on the positions
// the two swaps brought in-thread, and a record is a row of M N -- N first, then everything behind the last group.
static void qualify_lane_swap(const FastGroupBuilder &b, Stage &st) {
  const qmle_plan *p = b.p;
  const int T = b.T;
  st.lane_swap_last = st.lane_swap_cross = false;
  st.zreg_between.clear();
  std::memset(st.zreg_swap, 0, sizeof(st.zreg_swap));
  const int ng = st.fast_end - st.fast_begin;
  if (!(b.measured && st.zreg_ok && st.wave_private && st.dma_tables && ng >= 2)) return;
  const Group2 &gl = p->groups2[st.fast_end - 1];
  const Stage::FastGroupInfo &pi = st.fast_info[ng - 2], &li = st.fast_info[ng - 1];
  bool ok = gl.n_ops >= 1, straight = true, cross = true;  // which lane bit in-thread index 2 / 3 trades with
  uint32_t members = 0;
  for (int k = 0; k < (int)gl.n_ops && ok; ++k) {
    const LoweredOp &o = p->ops2[gl.op_begin + k];  // (t0: the in-thread index, which the dispatch code carries)
    ok = o.kind == LK_1Q && o.nc == 0 && !(o.flags & LF_PERMX) && (o.t0 == 2 || o.t0 == 3);
    if (!ok) break;
    const int pos = (int)li.bits[(int)o.t0];
    straight = straight && pos == (int)pi.thread_bits[o.t0 + 2];
    cross = cross && pos == (int)pi.thread_bits[7 - o.t0];
    members |= 1u << pos;
  }
  ok = ok && (straight || cross);
  cross = !straight;
  const std::vector<int8_t> &between = b.before_last.since;
  for (size_t i = 0; i + 1 < between.size() && ok; i += 2)
    if (members & ((1u << between[i + 1]) | (between[i] >= 0 ? 1u << between[i] : 0u))) ok = false;
  if (!ok) return;
  const LayoutMaps &m = b.maps, &nm = b.before_last;
  // in-thread index i = 2, 3 trades with lane bit lane_of(i)
  auto lane_of = [&](int i) { return cross ? 7 - i : i + 2; };
  for (int i = 0; i < 4; ++i) st.zreg_swap_bits[i] = (int8_t)(i < 2 ? (int)pi.bits[i] : (int)pi.thread_bits[lane_of(i)]);
  for (int t = 0; t < T - 4; ++t) st.zreg_swap_thread_bits[t] = pi.thread_bits[t];
  for (int i = 2; i < 4; ++i) st.zreg_swap_thread_bits[lane_of(i)] = (int8_t)pi.bits[i];
  const uint32_t cnst = m.M_lin(nm.Mconst) ^ m.Mconst;
  for (int j = 0; j < T; ++j) {
    uint32_t rec = ((cnst >> j) & 1u) << 15;
    for (int i = 0; i < 4; ++i) rec |= ((m.M_lin(nm.Mcol[(int)st.zreg_swap_bits[i]]) >> j) & 1u) << i;
    for (int t = 0; t < T - 4; ++t) rec |= ((m.M_lin(nm.Mcol[(int)st.zreg_swap_thread_bits[t]]) >> j) & 1u) << (4 + t);
    st.zreg_swap[j] = (uint16_t)rec;
  }
  st.zreg_between = between;
  st.lane_swap_last = true;
  st.lane_swap_cross = cross;
}

// measured: the stage qualifies for <Z> from the last group's registers (qualifies_for_register_measure).  Its X / CX
// that would hand a slot of one wave's slab to another wave -- the target's layout column holds one of the top
// T - 10 slot bits -- and whose bits no later op of the stage touches are kept back and applied behind the last group,
// where they only change the records (Stage::zreg); the groups in front then keep one partition of the tile among the
// waves and the walk needs no barrier between them (mark_wave_private_phases).
static void build_fast_groups(qmle_plan *p, Stage &st, const std::vector<LoweredOp> &src,
                              uint32_t zin_local, bool measured) {
  st.fast_ok = false;
  st.fast_begin = st.fast_end = (int)p->groups2.size();
  st.fast_info.clear();
  st.slab_load = st.wave_private = st.dma_tables = st.lane_swap_last = st.lane_swap_cross = false;
  st.sync_tile_end = true;
  const int T = st.T;
  if (T < kFastMinT || T > kFastMaxT || (p->flags & QMLE_PLAN_NO_REGTILE)) return;
  for (const LoweredOp &o : src)
    if (o.kind != LK_1Q || o.nc > 1) return;
  FastGroupBuilder b(p, st, src, zin_local, measured);
  b.form_groups();
  st.zreg_after = b.maps.since;
  emit_relayout(b);
  emit_zreg_records(b, st);
  // global byte offset of every lane's first float4 inside the tile: local index 2 t with its
  // bits deposited at the tile's global positions (bits below L are contiguous)
  st.fast_gtab = (uint32_t)p->tbl2.size();
  for (uint32_t t = 0; t < b.nt; ++t) {
    const uint32_t jl = 2u * t;
    uint32_t g = 0;
    for (int j = 0; j <= T - 4; ++j)
      if (jl & (1u << j)) g |= 1u << st.tile_bits[j];
    p->tbl2.push_back(g << 3);
  }
  st.fast_end = (int)p->groups2.size();
  st.fast_ok = true;
  mark_wave_private_phases(p, st, measured);
  qualify_lane_swap(b, st);
}

// Which wave touches which slot in every phase of the measuring walk, read off the tables as emitted; sets
// Group2::sync, Stage::slab_load / sync_tile_end / wave_private (Stage::fast_info) and emits the slab load map's
// global offsets.  The walk hands the last group's registers to the measurement, so no re-layout scatter is a phase.
static void mark_wave_private_phases(qmle_plan *p, Stage &st, bool measured) {
  const int T = st.T, ng = st.fast_end - st.fast_begin;
  if (!measured || ng <= 0 || T < 10) return;
  const uint32_t nt = 1u << (T - 4), size = 1u << T;
  auto staging = [&](bool slab) {  // a lane's 8 float4 = 16 slots (qmle_tile.hip, k_tile2)
    std::vector<uint8_t> own(size);
    for (uint32_t t = 0; t < nt; ++t)
      for (uint32_t u = 0; u < 8; ++u) {
        const uint32_t e = slab ? (2u * (t & 63u)) | (u << 7) | ((t >> 6) << 10) : (2u * t) | (u << (T - 3));
        own[swz(e)] = own[swz(e) ^ 1u] = (uint8_t)(t >> 6);
      }
    return own;
  };
  auto gather = [&](const Group2 &g) {
    std::vector<uint8_t> own(size);
    for (uint32_t t = 0; t < nt; ++t)
      for (int c = 0; c < 16; ++c) own[((p->tbl2[g.tbl + t] ^ g.off[c]) >> 3) & (size - 1u)] = (uint8_t)(t >> 6);
    return own;
  };
  std::vector<std::vector<uint8_t>> part;
  for (int g = 0; g < ng; ++g) part.push_back(gather(p->groups2[st.fast_begin + g]));
  st.slab_load = part[0] == staging(true);
  const std::vector<uint8_t> staged = staging(st.slab_load);
  bool any = false;
  for (int g = 0; g < ng; ++g) {
    const bool sync = part[g] != (g ? part[g - 1] : staged);
    p->groups2[st.fast_begin + g].sync = sync ? 1 : 0;
    any |= sync;
  }
  st.sync_tile_end = part[ng - 1] != staged;
  st.wave_private = !any && !st.sync_tile_end;
  if (st.slab_load) {
    st.fast_gtab_slab = (uint32_t)p->tbl2.size();
    for (uint32_t t = 0; t < nt; ++t) {
      const uint32_t jl = (2u * (t & 63u)) | ((t >> 6) << 10);
      uint32_t g = 0;
      for (int j = 0; j < T; ++j)
        if (jl & (1u << j)) g |= 1u << st.tile_bits[j];
      p->tbl2.push_back(g << 3);
    }
  }
  // LDS DMA in place of register staging (Stage::dma_tables): the wave that gathered a slot last stages it next, and
  // gathers it first.  The DMA's destination is lane-linear, so the swizzle goes on the source index (swz is its own
  // inverse and stays inside a 1 KiB piece): the per-lane part of it here, bits 3 and 4 of the piece's part as deltas.
  st.dma_tables = st.slab_load && !(p->groups2[st.fast_begin].sync & 1) && !st.sync_tile_end;
  if (st.dma_tables) {
    auto global_of = [&](uint32_t e) {
      uint32_t g = 0;
      for (int j = 0; j < T; ++j)
        if (e & (1u << j)) g |= 1u << st.tile_bits[j];
      return g << 3;
    };
    st.fast_gtab_dma = (uint32_t)p->tbl2.size();
    for (uint32_t t = 0; t < nt; ++t) p->tbl2.push_back(global_of(swz((2u * (t & 63u)) | ((t >> 6) << 10))));
    for (uint32_t k = 0; k < 4; ++k) st.dma_delta[k] = global_of(k << 3);
  }
}

// ---- unit-pivot forms of the fast tile path (FC_UDENSE / FC_UDIAG) ------------------------------
// A dense 2x2 on 16 amplitudes is 64 packed instructions in k_tile2, a quarter of which multiply by a number that
// can be factored out: U = pivot * U' with a literal 1 in U' costs 48.  A scalar commutes with every gate, so the
// pivots of a stage's unit-form ops are multiplied into ONE later gate of the same stage, the carrier (P U, plain
// form): the stage leaves the state it left before, up to rounding.  Per fast stage, over its ops2 stream in order:
//   * eligible: an uncontrolled dense or diagonal op whose source gates all come from the fixed / parametrised
//     unitary gate set (a caller's constant matrix need not be unitary: |pivot| >= 1 / sqrt 2 rests on that; a
//     controlled gate acts on half the amplitudes, where a factor is not a scalar);
//   * the last eligible dense op is the carrier, eligible ops in front of it take the unit form, eligible diagonal
//     ops behind it stay plain (their pivot, a phase, would have no carrier);
//   * a chain holds at most kMaxChainUnits unit-form ops: behind that the next eligible dense op is a carrier too.
// The records of unit-form ops and carriers are APPENDED to the matrix row (ops2[].mat_off; one build item per chain,
// BuildGroup::dim = kBuildChain); the plain records stay where every other reader finds them -- k_tile, k_direct_1q,
// k_reg_measure*, the product kernels, the adjoint sweep and the complex128 engine read dev_ops / lowered.
// what assign_product_forms needs to know about the ops of ops2: the 2x2 build group an eligible op's matrix comes from
// (-1: not eligible), what its ops2 record holds (ChainMember) and, for a carrier, the unit-form members of its chain
struct FastOpForms {
  std::vector<int> src_group;
  std::vector<uint16_t> role;
  std::vector<std::vector<int>> chain_units;  // per ops2 index of a carrier (empty elsewhere)
};
static void assign_unit_forms(qmle_plan *p, FastOpForms &forms) {
  forms.src_group.assign(p->ops2.size(), -1);
  forms.role.assign(p->ops2.size(), (uint16_t)CM_PLAIN);
  forms.chain_units.assign(p->ops2.size(), {});
  p->mat_floats_old = p->mat_floats;
  std::vector<int> group_at(p->mat_floats / 8 + 1, -1);  // plain record -> its 2x2 build group
  for (size_t g = 0; g < p->groups.size(); ++g)
    if (p->groups[g].dim == 2) group_at[p->groups[g].mat_off / 8] = (int)g;
  auto eligible = [&](const LoweredOp &o) {
    if (o.kind != LK_1Q || o.nc != 0) return false;
    const bool dense = o.pad < FC_CDENSE, diag = o.pad >= FC_DIAG && o.pad < FC_CDIAG;
    if (!dense && !diag) return false;
    const int g = o.mat_off / 8 < group_at.size() ? group_at[o.mat_off / 8] : -1;
    if (g < 0) return false;
    for (uint32_t k = p->groups[g].begin; k < p->groups[g].end; ++k)
      switch (p->build_ops[k].opcode) {
        case QMLE_OP_ID: case QMLE_OP_X: case QMLE_OP_Y: case QMLE_OP_Z: case QMLE_OP_H: case QMLE_OP_S:
        case QMLE_OP_RX: case QMLE_OP_RY: case QMLE_OP_RZ: case QMLE_OP_ROT: break;
        default: return false;
      }
    return true;
  };
  for (Stage &st : p->stages) {
    st.unit_form_ops.clear();
    st.scale_carriers.clear();
    if (st.kind != ST_TILE || !st.fast_ok || st.fast_end <= st.fast_begin) continue;
    const uint32_t ob = p->groups2[st.fast_begin].op_begin;
    uint32_t n_ops = 0;
    for (int g = st.fast_begin; g < st.fast_end; ++g) n_ops += p->groups2[g].n_ops;
    int last_dense = -1, n_elig = 0;
    std::vector<char> elig(n_ops, 0);
    for (uint32_t i = 0; i < n_ops; ++i) {
      elig[i] = eligible(p->ops2[ob + i]) ? 1 : 0;
      if (elig[i]) forms.src_group[ob + i] = group_at[p->ops2[ob + i].mat_off / 8];
      if (elig[i] && p->ops2[ob + i].pad < FC_CDENSE) last_dense = (int)i;
    }
    for (int i = 0; i <= last_dense; ++i) n_elig += elig[i];
    if (n_elig < 2) continue;
    std::vector<int> chain;  // unit-form members of the open chain (stream indices)
    auto close_chain = [&](int carrier) {
      if (chain.empty()) return;  // (nothing to carry: the op stays as it is)
      BuildGroup bg{(uint32_t)p->build_ops.size(), 0, p->mat_floats, kBuildChain};
      chain.push_back(carrier);
      for (size_t m = 0; m < chain.size(); ++m) {
        LoweredOp &o = p->ops2[ob + chain[m]];
        const BuildGroup src = p->groups[group_at[o.mat_off / 8]];
        for (uint32_t k = src.begin; k < src.end; ++k) {
          const BuildOp b = p->build_ops[k];
          p->build_ops.push_back(b);
        }
        const bool is_carrier = m + 1 == chain.size(), diag = o.pad >= FC_DIAG;
        BuildOp mark{};
        mark.opcode = kChainMark;
        mark.pad = is_carrier ? CM_CARRIER : diag ? CM_UNIT_DIAG : CM_UNIT_DENSE;
        mark.slot[0] = mark.slot[1] = mark.slot[2] = -1;
        mark.const_off = (int32_t)p->mat_floats;
        p->build_ops.push_back(mark);
        o.mat_off = p->mat_floats;
        p->mat_floats += 8;
        forms.role[ob + chain[m]] = mark.pad;
        if (is_carrier) {
          st.scale_carriers.push_back(chain[m]);
          for (size_t u = 0; u + 1 < chain.size(); ++u) forms.chain_units[ob + chain[m]].push_back((int)ob + chain[u]);
        } else {
          o.pad = (uint8_t)((diag ? FC_UDIAG : FC_UDENSE) + o.t0);
          st.unit_form_ops.push_back(chain[m]);
        }
      }
      bg.end = (uint32_t)p->build_ops.size();
      p->groups.push_back(bg);
      chain.clear();
    };
    for (int i = 0; i <= last_dense; ++i) {
      if (!elig[i]) continue;
      const bool dense = p->ops2[ob + i].pad < FC_CDENSE;
      if (i == last_dense) close_chain(i);
      else if ((int)chain.size() < kMaxChainUnits) chain.push_back(i);
      else if (dense) close_chain(i);
      // (else: a diagonal op behind a full chain stays plain)
    }
  }
}

// ---- product form of a Group2 ----------------------------------------------------------
// The uncontrolled one-qubit operators of a group sit on distinct in-thread bits and commute: the group applies their
// tensor product.  Each factors as M = g diag(1, l) [[c, -s], [s, c]] diag(1, r) with c, s >= 0 real and l, r, g / |g|
// unit phases; the right factors of the group multiply into one opening diagonal over the 16 amplitudes, the left
// factors and every scale into one closing diagonal, and what stays per gate is a REAL step, in which one packed FMA
// handles both halves of a complex amplitude: 16 packed instructions (c >= s) or 24 (c < s) where the unit-pivot form
// takes 48 (product_form_group, qmle_matrices.h; the kernel side: product_group, qmle_tile.hip).
// A group qualifies when it holds >= 2 ops, every one of them eligible for assign_unit_forms (plain, unit-form or
// carrier), no two on one bit.  Its record is APPENDED behind the unit-form records (Group2::prod_off); it factors the
// operators the ops2 records hold -- U / pivot, P U, U -- so that product-form and ordinary groups mix inside a stage
// and a chain's scaling stays what it was.  The ops2 records themselves stay: qmle_plan::mat_floats_unit is where they
// end, mat_floats the stride of the row.
static void assign_product_forms(qmle_plan *p, const FastOpForms &forms) {
  p->mat_floats_unit = p->mat_floats;
  for (Stage &st : p->stages) {
    if (st.kind != ST_TILE || !st.fast_ok) continue;
    for (int gi = st.fast_begin; gi < st.fast_end; ++gi) {
      Group2 &g = p->groups2[gi];
      if (g.n_ops < 2) continue;
      uint32_t bits = 0;
      bool ok = true;
      for (uint32_t i = g.op_begin; i < g.op_begin + g.n_ops && ok; ++i) {
        const LoweredOp &o = p->ops2[i];
        ok = forms.src_group[i] >= 0 && o.t0 >= 0 && o.t0 < 4 && !(bits & (1u << o.t0));
        if (ok) bits |= 1u << o.t0;
      }
      if (!ok) continue;
      BuildGroup bg{(uint32_t)p->build_ops.size(), 0, p->mat_floats, kBuildProduct};
      auto member = [&](int i, int bit) {
        const BuildGroup src = p->groups[forms.src_group[i]];
        for (uint32_t k = src.begin; k < src.end; ++k) {
          const BuildOp b = p->build_ops[k];
          p->build_ops.push_back(b);
        }
        BuildOp mark{};
        mark.opcode = kChainMark;
        mark.pad = forms.role[i];
        mark.slot[0] = mark.slot[1] = mark.slot[2] = -1;
        mark.const_off = bit;
        p->build_ops.push_back(mark);
      };
      for (uint32_t i = g.op_begin; i < g.op_begin + g.n_ops; ++i) {
        // (a carrier's P: the pivots of its chain's members in earlier groups, then of those in this one)
        for (int u : forms.chain_units[i])
          if ((uint32_t)u < g.op_begin) member(u, -1);
        member((int)i, (int)p->ops2[i].t0);
      }
      bg.end = (uint32_t)p->build_ops.size();
      p->groups.push_back(bg);
      g.prod_off = p->mat_floats;
      g.sync |= kGroupProduct | ((bits & 3u) ? 0 : kGroupProductLow1);
      p->mat_floats += kProductRecFloats;
    }
  }
}

// ---- product-form groups without closing diagonals -----------------------------------------
// A closing diagonal holds unit phases and the real scales the two-shear step leaves out.  Where nothing follows a
// group's wires but basis permutations and |amplitude|^2, the phases are invisible, and a rotation written as three
// shears has no scale: the record's measured mode (product_form_group) needs no closing diagonal.  kGroupClosingFree
// says a group MAY run that way -- in a run whose last stage this is and which ends in |amplitude|^2 only
// (measured_records_from, qmle_engine.hip); which mode a record is built in is decided per run.
//   Rule 1: every member's FastGroupBuilder::perm_tail holds.
//   Rule 2: the measured mode drops |g| per member, and the pivots of a unit-pivot chain cancel against its carrier's P
//           only when all of them are dropped: a chain with a member in a marked group has all its members in marked
//           groups (of the same stage: a chain never leaves its stage).  Iterated to the fixed point.
static void mark_closing_free_groups(qmle_plan *p, const FastOpForms &forms) {
  for (Stage &st : p->stages) {
    if (st.kind != ST_TILE || !st.fast_ok || st.fast_end <= st.fast_begin) continue;
    const uint32_t ob = p->groups2[st.fast_begin].op_begin;
    uint32_t oe = ob;
    std::vector<int> group_of;  // per op of the stage's stream
    for (int gi = st.fast_begin; gi < st.fast_end; ++gi) {
      Group2 &g = p->groups2[gi];
      bool ok = (g.sync & kGroupProduct) != 0;
      for (uint32_t i = g.op_begin; i < g.op_begin + g.n_ops; ++i) {
        ok = ok && p->ops2_perm_tail[i];
        group_of.push_back(gi);
      }
      oe += g.n_ops;
      if (ok) g.sync |= kGroupClosingFree;
    }
    auto marked = [&](uint32_t i) { return (p->groups2[group_of[i - ob]].sync & kGroupClosingFree) != 0; };
    for (bool changed = true; changed;) {
      changed = false;
      for (uint32_t c = ob; c < oe; ++c) {
        if (forms.chain_units[c].empty()) continue;
        bool any = marked(c), all = any;
        for (int u : forms.chain_units[c]) {
          any = any || marked((uint32_t)u);
          all = all && marked((uint32_t)u);
        }
        if (!any || all) continue;
        p->groups2[group_of[c - ob]].sync &= (uint8_t)~kGroupClosingFree;
        for (int u : forms.chain_units[c]) p->groups2[group_of[(uint32_t)u - ob]].sync &= (uint8_t)~kGroupClosingFree;
        changed = true;
      }
    }
  }
  // the builder reads the bit off the group's markers (BuildOp::pad2)
  std::vector<char> free_at(p->mat_floats / kProductRecFloats + 2, 0);  // (records are kProductRecFloats apart from mat_floats_unit on)
  for (const Group2 &g : p->groups2)
    if ((g.sync & kGroupProduct) && (g.sync & kGroupClosingFree)) free_at[(g.prod_off - p->mat_floats_unit) / kProductRecFloats] = 1;
  for (const BuildGroup &bg : p->groups) {
    if (bg.dim != kBuildProduct || !free_at[(bg.mat_off - p->mat_floats_unit) / kProductRecFloats]) continue;
    for (uint32_t k = bg.begin; k < bg.end; ++k)
      if (p->build_ops[k].opcode == kChainMark) p->build_ops[k].pad2 = 1;
  }
}

int stage_lane_runs(const Stage &st, int top, uint32_t off[4], uint32_t mask[4], uint32_t pos[4]) {
  int r = 0;
  for (int j = 0; j <= top && r <= 4;) {
    int len = 1;
    while (j + len <= top && st.tile_bits[j + len] == st.tile_bits[j] + len) ++len;
    if (r < 4) {
      off[r] = (uint32_t)j;
      mask[r] = (1u << len) - 1u;
      pos[r] = (uint32_t)st.tile_bits[j];
    }
    ++r;
    j += len;
  }
  for (int k = r < 4 ? r : 4; k < 4; ++k) off[k] = mask[k] = pos[k] = 0;
  return r <= 4 ? r : -1;
}

// ---- observable absorption ---------------------------------------------------------------
// Going backwards through the tape, a gate is absorbed iff it is a basis permutation with a
// LINEAR index map (CX, SWAP), a diagonal gate (phases drop out of |amplitude|^2) or the
// identity, and no later gate that stays in the circuit touches one of its wires.
static bool absorbable(uint16_t opcode) {
  switch (opcode) {
    case QMLE_OP_ID: case QMLE_OP_Z: case QMLE_OP_S: case QMLE_OP_RZ: case QMLE_OP_CZ:
    case QMLE_OP_CRZ: case QMLE_OP_CPHASE: case QMLE_OP_RZZ: case QMLE_OP_DIAG_ALL:
    case QMLE_OP_CX: case QMLE_OP_SWAP:
      return true;
    default:
      return false;
  }
}

void split_expval_tail(const std::vector<qmle_op> &ops, int n, std::vector<qmle_op> &kept,
                       std::vector<qmle_op> &absorbed) {
  kept.clear();
  absorbed.clear();
  std::vector<char> take(ops.size(), 0);
  uint32_t blocked = 0;  // wires a kept later gate acts on
  const uint32_t all = n >= 32 ? 0xffffffffu : ((1u << n) - 1u);
  for (size_t k = ops.size(); k-- > 0;) {
    const qmle_op &op = ops[k];
    uint32_t wires = 0;
    if (op.opcode == QMLE_OP_DIAG_ALL) wires = all;
    else
      for (int a = 0; a < 4 && op.wire[a] >= 0; ++a) wires |= 1u << op.wire[a];
    if (absorbable(op.opcode) && !(wires & blocked)) take[k] = 1;
    else blocked |= wires;
    if (blocked == all) break;  // nothing earlier can be absorbed
  }
  for (size_t k = 0; k < ops.size(); ++k) (take[k] ? absorbed : kept).push_back(ops[k]);
}

uint32_t pull_back_z(const std::vector<qmle_op> &absorbed, int wire) {
  uint32_t m = 1u << wire;
  for (size_t k = absorbed.size(); k-- > 0;) {
    const qmle_op &op = absorbed[k];
    if (op.opcode == QMLE_OP_CX) {            // Z_t -> Z_c Z_t, Z_c -> Z_c
      if (m & (1u << op.wire[1])) m ^= 1u << op.wire[0];
    } else if (op.opcode == QMLE_OP_SWAP) {
      const uint32_t a = (m >> op.wire[0]) & 1u, b = (m >> op.wire[1]) & 1u;
      if (a != b) m ^= (1u << op.wire[0]) | (1u << op.wire[1]);
    }
  }
  return m;
}

// ---- 1. validate + lower ---------------------------------------------------------------------------
// The per-op checks, in tape order: the first failing op decides the error code.
static int validate_tape(const qmle_plan *p) {
  const int n = p->n;
  for (const qmle_op &op : p->ops) {
    OpInfo info;
    if (!op_info(op.opcode, &info)) return QMLE_ERR_UNKNOWN_OP;
    int nw = 0;
    while (nw < 4 && op.wire[nw] >= 0) ++nw;
    if (op.opcode == QMLE_OP_DIAG_ALL) {
      // wires are implicitly 0..n-1 in order (operations.py:922-926)
      if (op.mat_off < 0 || (size_t)op.mat_off + (1ull << n) > p->consts.size())
        return QMLE_ERR_INVALID_ARG;
    } else {
      if (nw != info.n_wires) return QMLE_ERR_WIRE_COUNT;
      for (int a = 0; a < nw; ++a) {
        if (op.wire[a] >= n) return QMLE_ERR_WIRE_RANGE;
        for (int b = a + 1; b < nw; ++b)
          if (op.wire[a] == op.wire[b]) return QMLE_ERR_DUPLICATE_WIRES;
      }
      if (info.has_const) {
        const size_t need = op.opcode == QMLE_OP_MAT1 ? 8 : op.opcode == QMLE_OP_MAT2 ? 32 : 512;
        if (op.mat_off < 0 || (size_t)op.mat_off + need > p->consts.size())
          return QMLE_ERR_INVALID_ARG;
      }
    }
    for (int a = 0; a < info.n_params; ++a)
      if (op.slot[a] < 0 || op.slot[a] >= p->n_slots) return QMLE_ERR_SLOT_RANGE;
    if (op.opcode == QMLE_OP_MAT1_ROW || op.opcode == QMLE_OP_MAT2_ROW) {  // the matrix entries: consecutive columns
      const int need = op.opcode == QMLE_OP_MAT1_ROW ? 8 : 32;
      if ((long long)op.slot[0] + need > (long long)p->n_slots) return QMLE_ERR_SLOT_RANGE;
    }
  }
  return QMLE_OK;
}

constexpr uint8_t kLoweredDead = 255;  // LoweredOp::kind of an operator merged away during lowering

// One gate of a validated tape as a lowered operator on bit positions (wire w = position n - 1 - w); a dense
// operator's matrix offset is assigned when it is pushed.
static LoweredOp lowered_form(const qmle_op &op, int n) {
  auto pos = [n](int w) { return (int8_t)(n - 1 - w); };
  LoweredOp lo{};
  lo.t1 = lo.c0 = lo.c1 = -1;
  lo.slot = -1;
  lo.flags = is_diag_opcode(op.opcode) ? LF_DIAG : 0;
  if (op.opcode == QMLE_OP_X || op.opcode == QMLE_OP_CX || op.opcode == QMLE_OP_CCX)
    lo.flags |= LF_PERMX;
  if (op.opcode == QMLE_OP_CZ || op.opcode == QMLE_OP_CPHASE) lo.flags |= LF_PHASE;  // (operations.py:1100, 1171-1201)
  switch (op.opcode) {
    case QMLE_OP_DIAG_ALL:
      lo.kind = LK_DIAG_ALL;
      lo.t0 = 0;
      lo.mat_off = (uint32_t)op.mat_off;
      lo.slot = op.slot[0];
      break;
    case QMLE_OP_MAT4:
      lo.kind = LK_4Q;
      lo.t0 = pos(op.wire[0]); lo.t1 = pos(op.wire[1]);
      lo.c0 = pos(op.wire[2]); lo.c1 = pos(op.wire[3]);
      lo.nc = 0;
      lo.mat_off = (uint32_t)op.mat_off;  // const blob; permuted copy is made per stage
      break;
    case QMLE_OP_CX: case QMLE_OP_CY: case QMLE_OP_CZ: case QMLE_OP_CRX:
    case QMLE_OP_CRY: case QMLE_OP_CRZ: case QMLE_OP_CPHASE:
      lo.kind = LK_1Q; lo.nc = 1; lo.c0 = pos(op.wire[0]); lo.t0 = pos(op.wire[1]);
      break;
    case QMLE_OP_CCX:
      lo.kind = LK_1Q; lo.nc = 2; lo.c0 = pos(op.wire[0]); lo.c1 = pos(op.wire[1]);
      lo.t0 = pos(op.wire[2]);
      break;
    case QMLE_OP_CSWAP:
      lo.kind = LK_2Q; lo.nc = 1; lo.c0 = pos(op.wire[0]); lo.t0 = pos(op.wire[1]);
      lo.t1 = pos(op.wire[2]);
      break;
    case QMLE_OP_SWAP: case QMLE_OP_RXX: case QMLE_OP_RYY: case QMLE_OP_RZZ:
    case QMLE_OP_RZX: case QMLE_OP_MAT2: case QMLE_OP_MAT2_ROW:
      lo.kind = LK_2Q; lo.nc = 0; lo.t0 = pos(op.wire[0]); lo.t1 = pos(op.wire[1]);
      break;
    default:  // uncontrolled 1-qubit
      lo.kind = LK_1Q; lo.nc = 0; lo.t0 = pos(op.wire[0]);
      break;
  }
  return lo;
}

// What lower_tape keeps while it walks the tape.
struct Lowering {
  qmle_plan *p;
  std::vector<int> last_touch;                            // lowered index that last touched bit position b
  std::vector<std::vector<BuildOp>> group_ops;            // source gates per matrix
  std::vector<std::pair<uint32_t, uint32_t>> group_meta;  // (mat_off, dim)
  std::vector<int> group_of;                              // lowered index -> group

  explicit Lowering(qmle_plan *p_) : p(p_), last_touch(p_->n, -1) {}

  // a new operator behind everything lowered so far, made of the tape's gates `src`; -> its index
  int push(const LoweredOp &lo, std::vector<int> src) {
    const int idx = (int)p->lowered.size();
    const uint64_t m = op_mask(lo, p->n);
    for (int b = 0; b < p->n; ++b)
      if (m & bit(b)) last_touch[b] = idx;
    group_of.resize(idx + 1, -1);
    p->lowered.push_back(lo);
    p->lowered_src.push_back(std::move(src));
    return idx;
  }
  // gate `i` of the tape (`lo`, built by `bo`) multiplies onto operator `prev`: as U (x) I / I (x) U onto a 4x4
  // (BuildOp::pad = 1 / 2), else as a plain product (pad 0); `clear`: the flags a product cannot keep
  void multiply_onto(int prev, const LoweredOp &lo, BuildOp bo, int i, int pad, uint8_t clear) {
    LoweredOp &pl = p->lowered[prev];
    bo.pad = (uint16_t)pad;
    group_ops[group_of[prev]].push_back(bo);
    if (!(lo.flags & LF_DIAG)) pl.flags &= ~LF_DIAG;
    pl.flags &= ~clear;
    p->lowered_src[prev].push_back(i);
  }
  bool merge(const LoweredOp &lo, const BuildOp &bo, int i);
  void take_pending(LoweredOp &lo, std::vector<BuildOp> &taken, std::vector<int> &taken_src);
};

// Commutation-aware merge: an uncontrolled 1-q gate multiplies onto the previous uncontrolled 1-q matrix on the same
// wire if nothing touched that wire in between (gates on disjoint wires commute).
// Round 5: the same holds around an uncontrolled dense 4x4 (the Kraus superoperators of vec(rho) on [w, n + w],
// two-qubit Pauli rotations): a 1-q gate on one of its wires multiplies onto it as U (x) I / I (x) U
// (BuildOp::pad = 1 / 2), a 4x4 on the same ordered pair as a plain product, and a new 4x4 takes the
// pending 1-q matrices of its two wires with it (take_pending).  A noisy model's gate-channel-gate-channel run on one
// wire (U (x) conj U, superoperator, ...) becomes ONE 4x4 per sample.
bool Lowering::merge(const LoweredOp &lo, const BuildOp &bo, int i) {
  if (lo.nc != 0 || (lo.kind != LK_1Q && lo.kind != LK_2Q)) return false;
  const int prev = last_touch[lo.t0];
  if (prev < 0) return false;
  const LoweredOp &pl = p->lowered[prev];
  if (lo.kind == LK_1Q) {
    if (pl.kind == LK_1Q && pl.nc == 0 && pl.t0 == lo.t0) {
      multiply_onto(prev, lo, bo, i, 0, LF_PERMX);  // a product of gates is a general 2x2
      return true;
    }
    if (pl.kind == LK_2Q && pl.nc == 0 && (pl.t0 == lo.t0 || pl.t1 == lo.t0)) {
      multiply_onto(prev, lo, bo, i, pl.t0 == lo.t0 ? 1 : 2, 0);
      return true;
    }
    return false;
  }
  if (prev == last_touch[lo.t1] && pl.kind == LK_2Q && pl.nc == 0 && pl.t0 == lo.t0 && pl.t1 == lo.t1) {
    multiply_onto(prev, lo, bo, i, 0, 0);
    return true;
  }
  return false;
}

// the pending 1-q matrices a new uncontrolled 4x4 absorbs (they act first)
void Lowering::take_pending(LoweredOp &lo, std::vector<BuildOp> &taken, std::vector<int> &taken_src) {
  for (int side = 0; side < 2; ++side) {
    const int t = side == 0 ? lo.t0 : lo.t1;
    const int prev = last_touch[t];
    if (prev < 0) continue;
    LoweredOp &pl = p->lowered[prev];
    if (!(pl.kind == LK_1Q && pl.nc == 0 && pl.t0 == t)) continue;
    for (BuildOp b1 : group_ops[group_of[prev]]) {
      b1.pad = (uint16_t)(side + 1);
      taken.push_back(b1);
    }
    if (!(pl.flags & LF_DIAG)) lo.flags &= ~LF_DIAG;
    for (int s_ : p->lowered_src[prev]) taken_src.push_back(s_);
    group_ops[group_of[prev]].clear();  // (its matrix slot stays allocated, nothing builds or reads it)
    pl.kind = kLoweredDead;             // removed when the tape is through
  }
}

// Opcodes -> lowered operators (p->lowered, p->lowered_src) and the source gates of their matrices (p->build_ops,
// p->groups).  The tape has passed validate_tape.
static void lower_tape(qmle_plan *p) {
  const int n = p->n;
  p->lowered.clear(); p->lowered_src.clear(); p->build_ops.clear(); p->groups.clear();
  p->algo_bytes_per_state = 0;
  p->mat_floats = 0;
  const bool merging = !(p->flags & (QMLE_PLAN_NO_FUSION | QMLE_PLAN_NO_MERGE));
  Lowering lw(p);
  for (size_t i = 0; i < p->ops.size(); ++i) {
    const qmle_op &op = p->ops[i];
    p->algo_bytes_per_state += algo_bytes(op, n);
    if (op.opcode == QMLE_OP_ID) continue;  // identity: nothing to do
    LoweredOp lo = lowered_form(op, n);
    if (lo.kind == LK_DIAG_ALL || lo.kind == LK_4Q) {  // (their numbers come from the const blob: no build group)
      lw.push(lo, {(int)i});
      continue;
    }
    BuildOp bo{};
    bo.opcode = op.opcode;
    for (int a = 0; a < 3; ++a) bo.slot[a] = op.slot[a];
    bo.const_off = op.mat_off;
    if (merging && lw.merge(lo, bo, (int)i)) continue;
    std::vector<BuildOp> taken;
    std::vector<int> taken_src;
    if (merging && lo.kind == LK_2Q && lo.nc == 0) lw.take_pending(lo, taken, taken_src);
    const uint32_t dim = lo.kind == LK_2Q ? 4u : 2u;
    lo.mat_off = p->mat_floats;
    p->mat_floats += dim * dim * 2;
    taken.push_back(bo);
    taken_src.push_back((int)i);
    std::sort(taken_src.begin(), taken_src.end());
    const int idx = lw.push(lo, taken_src);
    lw.group_of[idx] = (int)lw.group_ops.size();
    lw.group_ops.push_back(taken);
    lw.group_meta.push_back({lo.mat_off, dim});
  }
  size_t w = 0;  // drop the 1-q operators a 4x4 absorbed
  for (size_t r = 0; r < p->lowered.size(); ++r) {
    if (p->lowered[r].kind == kLoweredDead) continue;
    if (w != r) {
      p->lowered[w] = p->lowered[r];
      p->lowered_src[w] = std::move(p->lowered_src[r]);
    }
    ++w;
  }
  p->lowered.resize(w);
  p->lowered_src.resize(w);
  // flatten the per-matrix source lists (tape order inside each group)
  for (size_t g = 0; g < lw.group_ops.size(); ++g) {
    if (lw.group_ops[g].empty()) continue;
    BuildGroup bg{(uint32_t)p->build_ops.size(), 0, lw.group_meta[g].first, lw.group_meta[g].second};
    for (const BuildOp &b : lw.group_ops[g]) p->build_ops.push_back(b);
    bg.end = (uint32_t)p->build_ops.size();
    p->groups.push_back(bg);
  }
}

// ---- 1b. low bit positions first ---------------------------------------------
// Gates that share no wire commute: among the gates that are ready (no earlier gate on any
// of their wires pending) take the one whose highest bit position is lowest.  The passes
// then work their way up from the low bits, and a run from |0..0> keeps its known-zero
// bits at the TOP: the amplitudes that can be non-zero stay one contiguous block (the
// measuring pass of K2 reads 8 MiB in one piece instead of 128-byte runs every 2 KiB).
static void reorder_low_bits_first(qmle_plan *p) {
  const int n = p->n;
  const size_t nl = p->lowered.size();
  if ((p->flags & (QMLE_PLAN_NO_FUSION | QMLE_PLAN_TAPE_ORDER)) || nl <= 1 || nl > 16384) return;
  std::vector<std::vector<int>> queue(n);  // per bit: ops touching it, tape order
  std::vector<size_t> head(n, 0);
  std::vector<uint64_t> masks(nl);
  for (size_t i = 0; i < nl; ++i) {
    masks[i] = op_mask(p->lowered[i], n);
    for (int b = 0; b < n; ++b)
      if (masks[i] & bit(b)) queue[b].push_back((int)i);
  }
  std::vector<std::pair<int, int>> heap;  // (highest bit, index), min-heap
  const std::greater<std::pair<int, int>> cmp;
  std::vector<char> queued(nl, 0);
  auto push_if_ready = [&](int i) {  // ready: at the head of the queue of every bit it touches
    if (queued[i]) return;
    for (int b = 0; b < n; ++b)
      if ((masks[i] & bit(b)) && queue[b][head[b]] != i) return;
    queued[i] = 1;
    heap.push_back({63 - __builtin_clzll(masks[i] ? masks[i] : 1ull), i});
    std::push_heap(heap.begin(), heap.end(), cmp);
  };
  for (size_t i = 0; i < nl; ++i) push_if_ready((int)i);
  std::vector<int> order;
  order.reserve(nl);
  while (!heap.empty()) {
    std::pop_heap(heap.begin(), heap.end(), cmp);
    const int i = heap.back().second;
    heap.pop_back();
    order.push_back(i);
    for (int b = 0; b < n; ++b)
      if (masks[i] & bit(b)) ++head[b];
    for (int b = 0; b < n; ++b)
      if ((masks[i] & bit(b)) && head[b] < queue[b].size()) push_if_ready(queue[b][head[b]]);
  }
  if (order.size() != nl) return;
  std::vector<LoweredOp> lo2(nl);
  std::vector<std::vector<int>> src2(nl);
  for (size_t k = 0; k < nl; ++k) {
    lo2[k] = p->lowered[order[k]];
    src2[k] = std::move(p->lowered_src[order[k]]);
  }
  p->lowered.swap(lo2);
  p->lowered_src.swap(src2);
}

// ---- 3. schedule into stages (for one tile geometry) ---------------------------
// A schedule candidate: the tile geometry (T tile positions, the lowest L of them contiguous) and what varies it.
// lazy: X / CX whose wires are not in the tile yet wait (the fast tile path folds them into
// the LDS layout for free, so they should never claim a tile bit a dense gate could use);
// whatever room is left after the first sweep is filled by a second, plain greedy sweep.
// HE layer at n = 24: dense gates per pass 12/7/5 -> 12/8/4, the measuring pass drops from
// two register-tile groups to one.
// carry >= 0: every tile after the first also holds bit position `carry` (position 6 = byte
// address bit 9: a read+write pass whose tile holds it moves two 128-byte rows 512 B apart with
// every load / store instruction and runs 12-15 % faster -- 51 -> 44 us per state at n = 24,
// profiles/r03_rw_tile_bits.txt; the price is one of the tile's 8 free positions).
// T_first > T: the first stage of a run from |0..0> computes ONE tile per state (everything else
// is zeros whatever the tile size), so it may stage up to 2^14 amplitudes at no cost in traffic.
// top_first (round 5, tuner candidates only): the first stage of a run from |0..0> -- ONE tile per state wherever
// that tile sits -- takes the TOP T_first positions instead of the low ones: every gate that lives inside that
// window runs on one tile per state, and what is left (the low positions plus whatever a deferred gate reaches
// up to) is scheduled as usual, on tiles with long contiguous rows.  The n = 24 headline layer: {10..23} first,
// then ONE measuring pass on {0..10, 23} -- two passes where the low-first schedule needs three.  The tile is a
// contiguous run of positions (Stage::shift): local index << shift is the address, no rows, no LUT.
// Such a schedule trades an HBM pass for arithmetic in the passes that are left: fewer bytes, less time, a
// lower fraction of the HBM roofline.
enum ScheduleVariant : int {
  SV_PLAIN = 0,             // the round-2 schedules
  SV_WIDE_FIRST = 1,        // wide first stage
  SV_CARRY_WIDE_FIRST = 2,  // position 6 carried + wide first stage
  SV_CARRY = 3,             // position 6 carried
  SV_TOP_FIRST = 4,         // first tile of 2^14 amplitudes on the TOP positions (all-live runs from |0..0>)
  kScheduleVariants = 5
};
constexpr int kGeometries[][2] = {{13, 7}, {13, 5}, {12, 4}, {13, 4}, {12, 5}, {13, 6}};  // (T, L)
constexpr int kNumGeometries = (int)(sizeof(kGeometries) / sizeof(kGeometries[0]));
constexpr int kCarriedPosition = 6;
struct ScheduleCandidate {
  int T, L;
  bool lazy;
  int carry;
  int T_first;
  bool top_first;
  int variant;
};
// Candidate number k (qmle_plan::chosen_candidate, QMLE_FORCE_CAND) = geometry x [eager, lazy CX] x variant, the
// geometry running fastest.  Ties between candidates keep the lower number.
constexpr int kCandidatesPerVariant = 2 * kNumGeometries;
constexpr int kNumCandidates = kCandidatesPerVariant * kScheduleVariants;
static int variant_of(int k) { return k / kCandidatesPerVariant; }
static ScheduleCandidate candidate_of(int k) {
  const int g = k % kNumGeometries, v = variant_of(k);
  const bool wide = v == SV_WIDE_FIRST || v == SV_CARRY_WIDE_FIRST || v == SV_TOP_FIRST;
  const bool carried = v == SV_CARRY_WIDE_FIRST || v == SV_CARRY;
  return {kGeometries[g][0], kGeometries[g][1], (k / kNumGeometries) % 2 != 0, carried ? kCarriedPosition : -1,
          wide ? kLdsMaxQubits : 0, v == SV_TOP_FIRST, v};
}

static inline int popc(uint64_t x) { return __builtin_popcountll(x); }
static inline uint64_t all_positions(int n) { return n >= 64 ? ~0ull : bit(n) - 1; }

// One run of schedule_stages: the candidate, and how far the lowered operators have been placed.
struct ScheduleRun {
  qmle_plan *p;
  ScheduleCandidate c;  // (T and L clamped to the register)
  int pad_high;         // QMLE_PAD_HIGH / qmle_plan::pad_high
  std::vector<char> done;
  size_t n_done = 0;
  uint32_t zeros;  // known-zero positions so far (|0..0> start)
  bool is_last(const std::vector<int> &members) const { return n_done + members.size() == p->lowered.size(); }
};

// Members of a top-first first stage on the window Q of the top T positions: every operator that lives inside it and
// has no operator in front of it that does not.  false: nothing lives up there (or everything does: one stage,
// nothing to gain).
static bool select_top_window(const qmle_plan *p, int T, std::vector<int> &members, uint64_t &Q) {
  const int n = p->n;
  const size_t nl = p->lowered.size();
  const uint64_t all_mask = all_positions(n), W = all_mask & ~(bit(n - T) - 1);
  uint64_t blocked = 0;
  for (size_t i = 0; i < nl; ++i) {
    const LoweredOp &o = p->lowered[i];
    const uint64_t m = op_mask(o, n);
    if (o.kind == LK_DIAG_ALL || (m & blocked) || (m & ~W)) blocked |= m;
    else members.push_back((int)i);
    if ((blocked & all_mask) == all_mask) break;
  }
  if (members.empty() || members.size() == nl) {
    members.clear();
    return false;
  }
  Q = W;
  return true;
}

// Members of a tile of T positions behind the operators placed so far, `first` the first pending one (no DIAG_ALL):
// greedy sweeps over the pending operators, the first of them lazy when the candidate says so.  Q: the positions the
// tile must hold; stageL: its contiguous low positions (fewer than the candidate's when the first operator needs room).
static void select_greedy(const ScheduleRun &r, size_t first, int T, std::vector<int> &members, uint64_t &Q, int &stageL) {
  const qmle_plan *p = r.p;
  const int n = p->n, carry = r.c.carry;
  const bool lazy = r.c.lazy, no_fusion = (p->flags & QMLE_PLAN_NO_FUSION) != 0;
  const size_t nl = p->lowered.size();
  const uint64_t all_mask = all_positions(n);
  // first pending op decides whether the default low-bit count fits
  const uint64_t fm = op_mask(p->lowered[first], n);
  while (stageL > 1 && popc((bit(stageL) - 1) | fm) > T) --stageL;
  Q = bit(stageL) - 1;
  if (carry >= stageL && carry < n && !p->stages.empty() && popc(Q | fm | bit(carry)) <= T) Q |= bit(carry);
  std::vector<char> taken;
  if (lazy) taken.assign(nl, 0);
  for (int sweep = lazy ? 0 : 1; sweep < 2; ++sweep) {
    uint64_t blocked = 0;
    for (size_t i = first; i < nl; ++i) {
      if (r.done[i] || (lazy && taken[i])) continue;
      const LoweredOp &o = p->lowered[i];
      const uint64_t m = op_mask(o, n);
      const bool wait = sweep == 0 && o.kind == LK_1Q && o.nc <= 1 && (o.flags & LF_PERMX) &&
                        (m & ~Q) != 0;
      if (o.kind == LK_DIAG_ALL || (m & blocked)) {
        blocked |= m;
      } else if (!wait && popc(Q | m) <= T) {
        Q |= m;
        members.push_back((int)i);
        if (lazy) taken[i] = 1;
        if (no_fusion) break;
      } else {
        blocked |= m;
      }
      if ((blocked & all_mask) == all_mask) break;
    }
    if (popc(Q) >= T) break;
  }
  // (an op taken by the second sweep never shares a wire with a LATER op of the first: that
  // one would have been blocked behind it -- so index order is a valid execution order)
  if (lazy) std::sort(members.begin(), members.end());
}

// A stage of one operator `m0` that the streaming kernel (k_direct_1q) runs, without a tile.
// a control on bits 1..3 selects 16/32/64-byte runs inside every 128-byte line: the
// streaming kernel would move whole lines for half the work (measured 2-4x slower
// than a tile pass at n = 28), so those go through the LDS tile instead
// (round 2: with the target on bits 1..6 too, the lane-exchange mode of the streaming
// kernel takes those controls: k_direct_1q mode 7)
static bool runs_direct(const qmle_plan *p, const LoweredOp &m0) {
  if (p->whole_state_lds || (p->flags & QMLE_PLAN_FORCE_TILE) || m0.kind != LK_1Q) return false;
  return m0.nc == 0 ||
         (m0.nc == 1 && (m0.c0 == 0 || m0.c0 >= 4 ||
                         (!(m0.flags & LF_DIAG) && p->n >= 14 && m0.t0 >= 1 && m0.t0 <= 6) ||
                         // a controlled PHASE rewrites the |11> quarter only (k_direct_1q mode 9):
                         // with the target above the line that is half the lines, not all of them
                         ((m0.flags & LF_PHASE) && m0.t0 >= 4)));
}

// The tile of a stage: the positions Q its members need, padded to T, as tile_bits / outer_bits, and the members
// with tile-local positions at the end of dev_ops.
static void place_tile(const ScheduleRun &r, Stage &st, const std::vector<int> &members, uint64_t Q, int T, int stageL,
                       bool top_stage) {
  qmle_plan *p = r.p;
  const int n = p->n, carry = r.c.carry;
  const bool last = !p->stages.empty() && r.is_last(members);  // the last stage of several
  // pad the tile with the lowest free bit positions
  // (tuning: QMLE_PAD_HIGH=1 pads the LAST stage from the top instead)
  if (r.pad_high && last) {
    if (carry >= stageL && carry < n && (Q & bit(carry))) {  // the carried position serves read+write passes
      uint64_t need = 0;
      for (int mi : members) need |= op_mask(p->lowered[mi], n);
      if (!(need & bit(carry))) Q &= ~bit(carry);
    }
    if (r.pad_high >= 2 && popc(Q) < T) Q |= bit(r.pad_high);  // (one chosen low position)
    for (int b = n - 1; b >= 0 && popc(Q) < T; --b) Q |= bit(b);
  }
  // The LAST stage of a 2^13-tile schedule whose gates need <= 12 positions takes a 2^12 tile: five 32 KiB
  // workgroups per CU overlap their loads and their groups where two 64 KiB ones do not (the measuring pass
  // of the 4-layer n = 24 model: DESIGN 9e, profiles/r05_small_last_tile_ab.txt)
  int Tpad = T;
  if (T == 13 && last && popc(Q) <= 12 && !(p->flags & QMLE_PLAN_NO_FUSION)) Tpad = 12;
  for (int b = 0; b < n && popc(Q) < Tpad; ++b) Q |= bit(b);
  st.T = popc(Q);
  int nt = 0, no = 0;
  int8_t local_of[64];
  for (int b = 0; b < n; ++b) {
    if (Q & bit(b)) { local_of[b] = (int8_t)nt; st.tile_bits[nt++] = (int8_t)b; }
    else { local_of[b] = -1; st.outer_bits[no++] = (int8_t)b; }
  }
  // contiguous low run actually present
  int run = 0;
  while (run < st.T && st.tile_bits[run] == run) ++run;
  st.L = run < 1 ? 1 : run;
  if (top_stage) {  // a contiguous run of positions that does not start at 0: address = local index << shift
    st.shift = n - st.T;
    st.L = st.T;
  }
  for (int mi : members) {
    LoweredOp o = p->lowered[mi];
    if (o.kind != LK_DIAG_ALL) {
      o.t0 = local_of[(int)o.t0];
      if (o.t1 >= 0) o.t1 = local_of[(int)o.t1];
      if (o.c0 >= 0) o.c0 = local_of[(int)o.c0];
      if (o.c1 >= 0) o.c1 = local_of[(int)o.c1];
    }
    p->dev_ops.push_back(o);
    p->dev_src.push_back(single_src(p, mi));
  }
}

// The members leave the pending set: the positions they mix, the tape's gates they cover, their SURVEY 8-d bytes.
static void record_members(ScheduleRun &r, Stage &st, const std::vector<int> &members) {
  const qmle_plan *p = r.p;
  for (int mi : members) {
    r.done[mi] = 1;
    ++r.n_done;
    const LoweredOp &lo = p->lowered[mi];  // global positions
    if (lo.kind == LK_4Q) {
      st.touched |= (1u << lo.t0) | (1u << lo.t1) | (1u << lo.c0) | (1u << lo.c1);
    } else if (lo.kind != LK_DIAG_ALL && !(lo.flags & LF_DIAG)) {
      st.touched |= 1u << lo.t0;  // controls keep their known-zero status
      if (lo.t1 >= 0) st.touched |= 1u << lo.t1;
    }
    for (int s : p->lowered_src[mi]) {
      st.src_ops.push_back(s);
      st.algo_bytes_per_state += algo_bytes(p->ops[s], p->n);
    }
  }
}

static void push_stage(ScheduleRun &r, Stage &st) {  // (Stage::zero_in: the known zeros along the execution order)
  st.zero_in = r.zeros;
  r.zeros &= ~st.touched;
  r.p->stages.push_back(st);
}

static void push_diag_all_stage(ScheduleRun &r, size_t i) {  // a full-register diagonal is a stage of its own
  qmle_plan *p = r.p;
  Stage st;
  st.kind = ST_DIAG_ALL;
  st.op_begin = (int)p->dev_ops.size();
  p->dev_ops.push_back(p->lowered[i]);
  p->dev_src.push_back(single_src(p, i));
  st.op_end = (int)p->dev_ops.size();
  st.src_ops = p->lowered_src[i];
  r.done[i] = 1;
  ++r.n_done;
  push_stage(r, st);
}

// What a stage's neighbours and its known-zero input decide: Stage::next_tile, Stage::product_ok, fold_groups.
static void mark_known_zeros(qmle_plan *p) {
  p->fold_groups = 0;
  for (size_t si = 0; si < p->stages.size(); ++si) {
    Stage &st = p->stages[si];
    st.next_tile = si + 1 < p->stages.size() && p->stages[si + 1].kind == ST_TILE;
    st.product_ok = false;
    if (st.kind != ST_TILE || si == 0 || st.grp_end <= st.grp_begin || st.T < 8) continue;
    uint32_t seen = 0;
    bool ok = true;
    for (int g = st.grp_begin; g < st.grp_end && ok; ++g) {
      const OpGroup &og = p->op_groups[g];
      ok = og.kind == GK_REG4;
      for (int j = 0; j < 4 && ok; ++j) {
        const uint32_t lb = 1u << og.bits[j];
        ok = !(seen & lb) && ((st.zero_in >> st.tile_bits[og.bits[j]]) & 1u);
        seen |= lb;
      }
    }
    st.product_ok = ok;
    if (ok && st.grp_end - st.grp_begin > p->fold_groups) p->fold_groups = st.grp_end - st.grp_begin;
  }
}

// The lowered operators as HBM passes under candidate `c`: whatever an earlier candidate left in the plan goes.
static void schedule_stages(qmle_plan *p, ScheduleCandidate c, int pad_high) {
  const int n = p->n;
  if (p->whole_state_lds) c.T = n;
  if (c.T > kLdsMaxQubits) c.T = kLdsMaxQubits;
  if (c.T > n) c.T = n;
  if (c.L > c.T) c.L = c.T;
  if (c.L < 1) c.L = 1;
  p->tile_T = c.T;
  p->tile_L = c.L;
  p->stages.clear();
  p->dev_ops.clear();
  p->dev_src.clear();
  p->op_groups.clear();
  p->ops2.clear();
  p->ops2_perm_tail.clear();
  p->groups2.clear();
  p->tbl2.clear();
  p->consts.resize(p->n_user_consts);  // drop permuted-matrix copies of a previous candidate
  const size_t nl = p->lowered.size();
  ScheduleRun r{p, c, pad_high, std::vector<char>(nl, 0), 0, n >= 32 ? ~0u : ((1u << n) - 1u)};
  const bool top_first = c.top_first && !p->whole_state_lds && n <= 28 &&
                         !(p->flags & (QMLE_PLAN_NO_FUSION | QMLE_PLAN_FORCE_TILE));
  while (r.n_done < nl) {
    std::vector<int> members;
    uint64_t Q = 0;
    int stageL = c.L, T = c.T;
    if (!p->whole_state_lds && p->stages.empty() && c.T_first > c.T)
      T = std::max(c.T, std::min(std::min(c.T_first, kLdsMaxQubits), n - 1));
    const bool top_stage = top_first && p->stages.empty() && T < n && select_top_window(p, T, members, Q);
    if (!top_stage && p->whole_state_lds) {
      for (size_t i = 0; i < nl; ++i) members.push_back((int)i);
      Q = all_positions(n);
    } else if (!top_stage) {
      size_t first = 0;
      while (r.done[first]) ++first;
      if (p->lowered[first].kind == LK_DIAG_ALL) {
        push_diag_all_stage(r, first);
        continue;
      }
      select_greedy(r, first, T, members, Q, stageL);
    }
    Stage st;
    st.L = stageL;
    st.op_begin = (int)p->dev_ops.size();
    if (!top_stage && members.size() == 1 && runs_direct(p, p->lowered[members[0]])) {
      st.kind = ST_DIRECT;
      p->dev_ops.push_back(p->lowered[members[0]]);
      p->dev_src.push_back(single_src(p, members[0]));
    } else {
      st.kind = ST_TILE;
      place_tile(r, st, members, Q, T, stageL, top_stage);
    }
    st.op_end = (int)p->dev_ops.size();
    st.n_tile_ops = st.op_end - st.op_begin;
    if (st.kind == ST_TILE) {
      const std::vector<LoweredOp> tile_local(p->dev_ops.begin() + st.op_begin, p->dev_ops.begin() + st.op_end);
      // (what qualifies_for_register_measure will ask of the finished plan; r.zeros is this stage's zero_in)
      const bool measured = placed_for_register_measure(p, st, r.zeros, p->stages.empty(), r.is_last(members));
      build_fast_groups(p, st, tile_local, gather_bits(r.zeros, st.tile_bits, st.T), measured);
      group_stage_ops(p, st);
    }
    record_members(r, st, members);
    push_stage(r, st);
  }
  if (p->whole_state_lds && p->stages.empty()) {
    // empty circuit: still need one stage to produce |0...0>
    Stage st;
    st.kind = ST_TILE;
    st.T = n;
    st.L = c.L;
    for (int b = 0; b < n; ++b) st.tile_bits[b] = (int8_t)b;
    push_stage(r, st);
  }
  mark_known_zeros(p);
}

// ---- pass-cost model ----------------------------------------------------------------------------
// Fast kernel (k_tile2), round-3 model, fitted to per-pass HIP-event times of 1- and 4-layer
// circuits at n = 24 with and without their gate groups (profiles/r03_pass_model.txt): a pass
// takes the LONGER of its memory time and its compute time plus a sixth of the shorter one.
//   memory: 19.5 us write-only, 21 read-only, 50 read+write (5.4 TB/s: the mix costs);
//   a read+write pass whose every load / store instruction spans positions 6 and 13 (byte
//   address bits 9 and 16) and no other position below 8 -- a wave's 8 rows of 128 B are
//   the tile's three lowest high positions -- runs 15 % faster (51.3 -> 43.3 us, K2 pass
//   2; 54 -> 45 in the bare pass for every tile {6, 13, x >= 8, ...} and for no other pair
//   tried); every pair of high positions 8 apart costs ~4.5 us (54 -> 71 for {12-15,
//   20-23}).  The HBM channel hash behind both is not documented: modelled as measured.
//   compute: 5 + 9.5 per register-tile group, + 10 for the <Z> sums of a measuring pass.
// rd, wr, tiles: the fractions of the state the pass reads, writes and computes.
static double fast_pass_cost(const qmle_plan *p, const Stage &st, bool first, bool last, double rd, double wr,
                             double tiles) {
  double rw = (first ? 0.0 : 21.0 * rd) + (last ? 0.0 : 19.5 * wr);
  if (!first && !last) {
    rw += 9.5 * (rd < wr ? rd : wr);
    double shape = 0.0;
    if (st.L == 4 && st.T >= 12) {
      const int h0 = st.tile_bits[4], h1 = st.tile_bits[5], h2 = st.tile_bits[6];
      if (h0 == 6 && h1 >= 8 && (h1 == 13 || h2 == 13)) shape -= 7.5;
    }
    uint32_t hi = 0;
    for (int j = st.L; j < st.T; ++j) hi |= 1u << st.tile_bits[j];
    shape += 4.5 * __builtin_popcount(hi & (hi >> 8));
    rw += shape * (rd < wr ? rd : wr);
  }
  const double cmp = (5.0 + 9.5 * (st.fast_end - st.fast_begin) + (last ? 10.0 : 0.0)) * tiles;
  return 1.5 + 0.8 * std::ldexp(1.0, 24 - p->n) + (rw > cmp ? rw + cmp / 6.0 : cmp + rw / 6.0);
}

// pass-cost model (microseconds per state at n = 24; measured on MI355X, dense passes of 1-
// and 3-layer HE circuits, tools/stage_profile.py): a tile pass costs ~11 for its HBM round
// trip and ~25 per register-tile group (the gate arithmetic is what a pass is made of: 62 us
// with 2 groups, 125 with 5, 192 with 7); a direct single-gate pass ~33
// Known zeros scale both parts: a stage reads 2^-|zero_in| of the state, computes and (when
// the next stage is a tile stage) stores only the tiles whose outer bits are live.
static double schedule_cost(const qmle_plan *p) {
  const int n = p->n;
  const bool sparse_model = !(p->flags & QMLE_PLAN_NO_SPARSE);
  // the plan is only ever run from |0..0> (qmle_run_batch): set on the variants / children that
  // qmle_plan_create compiles for that purpose, never on a plan handed to qmle_apply_inplace
  const bool zero_run = (p->flags & QMLE_PLAN_INTERNAL_ZERO_RUN) != 0;
  double c = 0;
  for (size_t si = 0; si < p->stages.size(); ++si) {
    const Stage &st = p->stages[si];
    if (st.kind != ST_TILE) { c += 33.0; continue; }
    double rd = si == 0 ? 0.0 : 1.0, wr = 1.0, tiles = 1.0;
    if (sparse_model && st.zero_in) {
      tiles = std::ldexp(1.0, -__builtin_popcount(st.zero_in & outer_mask(st, n)));
      if (si > 0) rd = std::ldexp(1.0, -__builtin_popcount(st.zero_in));
      if (st.next_tile) wr = tiles;
    }
    // the first stage of a run from |0..0> runs its gates on one tile per state (the rest is a fill)
    if (si == 0 && zero_run && !sparse_model) tiles = std::ldexp(1.0, st.T - n);
    const bool last = si + 1 == p->stages.size();
    if (st.fast_ok) {
      c += fast_pass_cost(p, st, si == 0, last, rd, wr, tiles);
      continue;
    }
    const double mem = rd + (last ? 0.0 : wr);
    c += 2.0 + 0.8 * std::ldexp(1.0, 24 - n) + 6.0 * mem +
         25.0 * (st.grp_end - st.grp_begin) * tiles;
  }
  // a schedule that ends in a streaming pass leaves the measurement to a pass of its own (one
  // more read of the state), where a tile pass measures on the fly
  if (!p->stages.empty() && p->stages.back().kind != ST_TILE) c += 21.0;
  return c;
}

// May the search (or QMLE_FORCE_CAND, for a top-first candidate) take candidate `c`?
static bool candidate_allowed(const qmle_plan *p, const ScheduleCandidate &c, bool no_top) {
  const int n = p->n, v = c.variant;
  const bool sparse_model = !(p->flags & QMLE_PLAN_NO_SPARSE), zero_run = (p->flags & QMLE_PLAN_INTERNAL_ZERO_RUN) != 0;
  if (c.T >= n) return false;
  // (known-zero runs keep the round-2 schedules: their first passes are launch-bound special
  // kernels tuned for the (12, 4) geometry, and the wide first tile cost them 4-8 % at n = 24)
  if (v != SV_PLAIN && sparse_model) return false;
  if ((v == SV_WIDE_FIRST || v == SV_CARRY_WIDE_FIRST) && !zero_run) return false;
  if (c.carry >= 0 && (c.L != 4 || n < 16)) return false;
  if (v == SV_TOP_FIRST && (!zero_run || no_top || n < 16 || n > 28)) return false;
  return true;
}

// The schedule of the plan: the forced geometry, or the cheapest candidate of the pass-cost model (p->cand_ranking:
// every candidate with its cost), or the candidate the tuning switches force.
static void choose_schedule(qmle_plan *p) {
  const int n = p->n;
  const int forced_T = (int)((p->flags >> 8) & 0xff), forced_L = (int)((p->flags >> 16) & 0xff);
  const int pad_high = p->pad_high >= 0 ? p->pad_high
                       : std::getenv("QMLE_PAD_HIGH") ? atoi(std::getenv("QMLE_PAD_HIGH")) : 0;
  if (p->whole_state_lds || forced_T != 0 || forced_L != 0 || (p->flags & QMLE_PLAN_NO_FUSION)) {
    schedule_stages(p, {forced_T ? forced_T : kDefaultTileBits, forced_L ? forced_L : kDefaultLowBits, false, -1, 0,
                        false, SV_PLAIN}, pad_high);
    return;
  }
  // QMLE_NO_TOP_FIRST=1: the round-4 candidates only.
  const bool no_top = std::getenv("QMLE_NO_TOP_FIRST") != nullptr;  // (read per compile: bench.py's k2_three_pass leg)
  const bool zero_run = (p->flags & QMLE_PLAN_INTERNAL_ZERO_RUN) != 0;
  int best = 0;
  double best_cost = 1e300;
  p->cand_ranking.clear();
  for (int k = 0; k < kNumCandidates; ++k) {
    const ScheduleCandidate c = candidate_of(k);
    if (!candidate_allowed(p, c, no_top)) continue;
    schedule_stages(p, c, pad_high);
    if (c.top_first && (p->stages.empty() || p->stages[0].shift == 0)) continue;  // (no top-first stage came of it)
    const double cost = schedule_cost(p);
    p->cand_ranking.push_back({cost, k});
    // (the round-3 variants must win by 2 %: the model knows their effect from two circuits; a top-first schedule
    // by 5 % -- it wins by dropping a whole pass or not at all: K2 headline 58.2 against 92.5 predicted, 60.5 against
    // 88.5 ms measured)
    const int vb = variant_of(best);
    const double margin = c.variant == SV_TOP_FIRST ? (vb != SV_TOP_FIRST ? 0.95 : 1.0)
                                                    : (c.variant != SV_PLAIN && vb == SV_PLAIN ? 0.98 : 1.0);
    if (cost < best_cost * margin - 1e-9) { best_cost = cost; best = k; }
  }
  std::sort(p->cand_ranking.begin(), p->cand_ranking.end());
  // (tuning only: force one of the candidates to measure it against the model's choice)
  const int force = p->force_candidate >= 0 ? p->force_candidate
                    : std::getenv("QMLE_FORCE_CAND") ? atoi(std::getenv("QMLE_FORCE_CAND")) : -1;  // (read per compile: tools/cand_sweep.py)
  if (force >= 0 && force < kNumCandidates) {
    const ScheduleCandidate c = candidate_of(force);
    if ((c.variant != SV_TOP_FIRST || candidate_allowed(p, c, no_top)) && c.T < n && (c.variant == SV_PLAIN || zero_run))
      best = force;
  }
  schedule_stages(p, candidate_of(best), pad_high);
  p->chosen_candidate = best;
}

// ---- matrices no forward kernel reads --------------------------------------------------------
// An X / CX inside a register-tile group is a swap of amplitudes (reg_dispatch<2>, f_x / f_cx) or a
// change of the LDS layout map (build_fast_groups); its 2x2 matrix is never read by a tile pass.  The
// per-sample matrix builder spent 46 % of its groups on them in the Fourier-grid model (60 CX of 130
// groups, a fifth of a saturated 10-qubit batch with the rest of the builder).  The
// build groups are ordered needed-first; the forward engine builds [0, n_groups_needed), the adjoint
// sweep and the complex128 engine (which apply a CX through its matrix) all of them.
static void order_build_groups(qmle_plan *p) {
  std::vector<char> unread(p->mat_floats + 1, 0);
  for (const Stage &st : p->stages) {
    if (st.kind != ST_TILE || st.T < 4 || (p->flags & QMLE_PLAN_NO_REGTILE)) continue;  // (group_stage_ops: regs_ok)
    for (int i = st.op_begin; i < st.op_end; ++i) {
      const LoweredOp &o = p->dev_ops[i];
      if (o.kind == LK_1Q && o.nc <= 1 && (o.flags & LF_PERMX)) unread[o.mat_off] = 1;
    }
  }
  auto needed = [&](const BuildGroup &g) { return !(g.dim == 2 && unread[g.mat_off]); };
  std::stable_partition(p->groups.begin(), p->groups.end(), needed);
  p->n_groups_needed = 0;
  p->n_product_groups = 0;
  for (const BuildGroup &g : p->groups) {
    if (needed(g)) ++p->n_groups_needed;
    if (g.dim == kBuildProduct) ++p->n_product_groups;  // (appended last, and needed: they close the needed range)
  }
}

int compile_plan(qmle_plan *p) {
  const int n = p->n;
  if (n < 1 || n > QMLE_MAX_QUBITS) return QMLE_ERR_INVALID_ARG;
  const int rc = validate_tape(p);
  if (rc != QMLE_OK) return rc;
  lower_tape(p);
  reorder_low_bits_first(p);
  // ---- 2. choose regime ------------------------------------------------------
  const int forced_T = (int)((p->flags >> 8) & 0xff);
  p->whole_state_lds = (n <= kLdsMaxQubits) && !(p->flags & QMLE_PLAN_FORCE_GLOBAL) &&
                       (forced_T == 0 || forced_T >= n);
  if (!p->whole_state_lds && forced_T != 0 && forced_T < 4 && forced_T < n)
    return QMLE_ERR_INVALID_ARG;
  choose_schedule(p);
  p->model_cost = schedule_cost(p);
  FastOpForms forms;
  assign_unit_forms(p, forms);
  assign_product_forms(p, forms);
  mark_closing_free_groups(p, forms);
  order_build_groups(p);
  return QMLE_OK;
}

// HBM bytes per state a stage moves in a run from |0..0> (TM_STORE epilogue; a fused
// measurement in the last stage writes nothing): known-zero amplitudes are not read, tiles of
// zeros are not stored when the next stage is a tile stage (Stage::zero_in / next_tile).
static double stage_read_bytes(const qmle_plan *p, size_t si) {
  const Stage &st = p->stages[si];
  const double D = std::ldexp(1.0, p->n);
  const bool sparse = !(p->flags & QMLE_PLAN_NO_SPARSE);
  if (st.kind != ST_TILE) return st.kind == ST_DIRECT ? 0.5 * st.algo_bytes_per_state : 8.0 * D;
  if (si == 0) return 0.0;  // generated in LDS
  if (!sparse) return 8.0 * D;
  uint32_t z = st.zero_in;
  int nz = __builtin_popcount(z & ~1u);  // 16-byte loads: bit 0 rides along
  return 8.0 * std::ldexp(1.0, p->n - nz);
}
static double stage_write_bytes(const qmle_plan *p, size_t si) {
  const Stage &st = p->stages[si];
  const double D = std::ldexp(1.0, p->n);
  const bool sparse = !(p->flags & QMLE_PLAN_NO_SPARSE);
  if (st.kind != ST_TILE) return st.kind == ST_DIRECT ? 0.5 * st.algo_bytes_per_state : 8.0 * D;
  // (the plan's last batch run left out fills of zeros that were in memory already: what it wrote)
  if (si == 0 && p->last_run.stage0_written) return (double)p->last_run.stage0_written;
  if (!sparse || !st.next_tile) return 8.0 * D;
  return 8.0 * std::ldexp(1.0, p->n - __builtin_popcount(st.zero_in & outer_mask(st, p->n)));
}

bool qualifies_for_register_measure(const qmle_plan *p, size_t si) {
  const Stage &st = p->stages[si];
  if (st.kind != ST_TILE || !st.fast_ok || !st.zreg_ok) return false;
  return placed_for_register_measure(p, st, st.zero_in, si == 0, si + 1 == p->stages.size());
}

void stage_known_zeros(const qmle_plan *p, const Stage &st, uint32_t *local, uint32_t *outer) {
  *local = gather_bits(st.zero_in, st.tile_bits, st.T);
  *outer = gather_bits(st.zero_in, st.outer_bits, p->n - st.T);
}

// (known zeros inside the tile: the walk zero-fills and loads selectively)
bool walk_by_dma(const Stage &st, uint32_t zin_local) { return st.dma_tables && !zin_local; }

bool stages_by_dma(const qmle_plan *p, size_t si) {
  const Stage &st = p->stages[si];
  if (!qualifies_for_register_measure(p, si)) return false;
  uint32_t local = 0, outer = 0;
  if (!(p->flags & QMLE_PLAN_NO_SPARSE)) stage_known_zeros(p, st, &local, &outer);
  return walk_by_dma(st, local);
}

TileFamily expval_kernel_of(const qmle_plan *p, size_t si, bool sparse) {
  const Stage &st = p->stages[si];
  if (st.kind != ST_TILE || si == 0) return TF_TILE;
  if (st.grp_end - st.grp_begin != 1 || p->op_groups[st.grp_begin].kind != GK_REG4) return TF_TILE;
  if (st.T < 10 || st.T > 14 || st.T >= p->n || (st.op_end - st.op_begin) > 1000) return TF_TILE;
  const OpGroup &g = p->op_groups[st.grp_begin];
  int live_bits = 0;  // register bits that are not known-zero on input
  for (int j = 0; j < 4; ++j)
    live_bits += !(sparse && ((st.zero_in >> st.tile_bits[g.bits[j]]) & 1u));
  if (live_bits == 0 && p->n - st.T >= 5) return TF_REG_MEASURE_MONO;
  return live_bits <= 2 && g.n_ops > 0 ? TF_REG_MEASURE_FOLD : TF_REG_MEASURE;
}

// fp32 flops per state of the operators the plan really applies (after 1-qubit merging): a dense
// 2x2 costs 4 complex multiplies + 2 complex adds per amplitude pair = 14 per amplitude, a
// diagonal one 6, a permutation 0; a control halves the amplitudes touched.
static double plan_flops_per_state(const qmle_plan *p) {
  const double D = std::ldexp(1.0, p->n);
  double f = 0;
  for (const LoweredOp &op : p->lowered) {
    const double live = D / (double)(1u << op.nc);
    switch (op.kind) {
      case LK_1Q: f += (op.flags & LF_PERMX) ? 0.0 : (op.flags & LF_DIAG) ? 6.0 * live : 14.0 * live; break;
      case LK_2Q: f += 30.0 * live; break;
      case LK_DIAG_ALL: f += 6.0 * D; break;
      case LK_4Q: f += 126.0 * D; break;
    }
  }
  return f;
}

// the same count for the operators of one stage.  `live`: in a run from |0..0> with known-zero tracking, an
// operator is charged for the amplitudes that can be non-zero when it is applied (every known-zero position
// outside its own bits halves them; a known-zero CONTROL leaves nothing to do; a gate that is not diagonal takes its
// target out of the set) -- what the kernels skip at wave granularity; else nominal, the whole register.
static double stage_flops_per_state(const qmle_plan *p, const Stage &st, bool live_only) {
  // (the first stage of an all-live run from |0..0> computes ONE tile per state -- the rest is a fill)
  const bool one_tile = !p->stages.empty() && &st == &p->stages[0] && st.kind == ST_TILE && st.T < p->n &&
                        (p->flags & QMLE_PLAN_INTERNAL_ZERO_RUN) && (p->flags & QMLE_PLAN_NO_SPARSE);
  const double D = std::ldexp(1.0, one_tile ? st.T : p->n);
  double f = 0;
  const bool sparse = live_only && !(p->flags & QMLE_PLAN_NO_SPARSE);
  uint32_t Z = sparse ? st.zero_in : 0u;
  // bit indices of a tile stage's ops: GROUP-local (0..3) inside a register-tile group, else tile-local
  std::vector<const OpGroup *> group_of(st.op_end > st.op_begin ? st.op_end - st.op_begin : 0, nullptr);
  if (st.kind == ST_TILE)
    for (int g = st.grp_begin; g < st.grp_end; ++g) {
      const OpGroup &og = p->op_groups[g];
      if (og.kind != GK_REG4 && og.kind != GK_REG4X) continue;
      for (int k = 0; k < (int)og.n_ops; ++k) {
        const int idx = (int)og.op_begin + k - st.op_begin;
        if (idx >= 0 && idx < (int)group_of.size()) group_of[idx] = &og;
      }
    }
  const OpGroup *cur = nullptr;
  auto gpos = [&](int b) {
    if (st.kind != ST_TILE || b < 0) return b;
    const int local = cur ? (int)cur->bits[b & 3] : b;
    return (int)st.tile_bits[local];
  };
  for (int i = st.op_begin; i < st.op_end && i < (int)p->dev_ops.size(); ++i) {
    const LoweredOp &op = p->dev_ops[i];
    cur = group_of.empty() ? nullptr : group_of[i - st.op_begin];
    uint32_t own = 0, ctl = 0;
    if (op.kind != LK_DIAG_ALL) {
      own |= 1u << gpos(op.t0);
      if (op.t1 >= 0) own |= 1u << gpos(op.t1);
      if (op.kind == LK_4Q) { own |= 1u << gpos(op.c0); own |= 1u << gpos(op.c1); }
      else {
        if (op.nc >= 1) ctl |= 1u << gpos(op.c0);
        if (op.nc >= 2) ctl |= 1u << gpos(op.c1);
      }
    }
    double amps = D / (double)(1u << op.nc);
    if (Z & ctl) amps = 0.0;
    else amps /= (double)(1ull << __builtin_popcount(Z & ~own & ~ctl));
    switch (op.kind) {
      case LK_1Q: f += (op.flags & LF_PERMX) ? 0.0 : (op.flags & LF_DIAG) ? 6.0 * amps : 14.0 * amps; break;
      case LK_2Q: f += 30.0 * amps; break;
      case LK_DIAG_ALL: f += 6.0 * amps; break;
      case LK_4Q: f += 126.0 * amps; break;
    }
    if (op.kind == LK_DIAG_ALL || (op.kind == LK_1Q && (op.flags & LF_DIAG))) continue;
    Z &= ~own;  // mixed positions are live from here on
  }
  return f;
}

// The measuring walk of stage `s` in describe_plan's words.
static void describe_measuring(std::ostringstream &os, const qmle_plan *p, size_t s) {
  const Stage &st = p->stages[s];
  // <Z> from the last group's registers (k_tile2's multi-tile measuring walk): whether the stage QUALIFIES
  // (qualifies_for_register_measure: last of several, k_tile2 records, no known-zero tiles; what a run really did
  // is in the _last_run fields below), the records, and what they were derived from
  const bool from_regs = qualifies_for_register_measure(p, s);
  os << ",\"register_measure_qualifies\":" << (from_regs ? "true" : "false");
  // the measuring walk's barriers (Stage::fast_info): which load map it stages with, whether a barrier stays between
  // the last group and the next tile's staging, and whether none is left in the tile loop
  if (st.fast_ok)
    os << ",\"load_map\":\"" << (st.slab_load ? "slab" : "rows") << "\",\"sync_tile_end\":"
       << (st.sync_tile_end ? "true" : "false") << ",\"wave_private_walk\":" << (st.wave_private ? "true" : "false");
  // how the walk stages a tile (Stage::dma_tables) and, for the DMA form, its source map: the byte offset of work
  // item t's pair inside the tile (the table, and the runs the kernel takes instead when there are at most four,
  // applied to sw(2 lane | wave << 10)), XOR the delta of piece u & 3, plus the offset of u's three bits
  if (st.fast_ok) {
    const bool dma = stages_by_dma(p, s);
    os << ",\"staging\":\"" << (dma ? "dma" : "registers") << "\"";
    if (dma) {
      os << ",\"dma_deltas\":[" << st.dma_delta[0] << "," << st.dma_delta[1] << "," << st.dma_delta[2] << ","
         << st.dma_delta[3] << "],\"dma_lane_offsets\":[";
      for (uint32_t t = 0; t < (1u << (st.T - 4)); ++t) os << (t ? "," : "") << p->tbl2[st.fast_gtab_dma + t];
      uint32_t off[4], mask[4], pos[4];
      const int nr = stage_lane_runs(st, st.T - 1, off, mask, pos);
      os << "],\"dma_lane_runs\":";
      if (nr < 0) os << "null";
      else {
        os << "[";
        for (int r = 0; r < nr; ++r) os << (r ? "," : "") << "[" << off[r] << "," << mask[r] << "," << pos[r] << "]";
        os << "]";
      }
    }
  }
  // the last group through lane swaps (Stage::lane_swap_last; like the DMA form it rides on, a run also needs an input
  // without known zeros inside the tile): the records of the frame behind the swaps, the positions of its in-thread
  // bits and of its thread bits; the X / CX behind it: `measure_between` (between the last two groups), then
  // `measure_after`
  const bool lane_swap = walk_by_lane_swap(st, stages_by_dma(p, s));
  os << ",\"last_group_lane_swap\":" << (lane_swap ? "true" : "false");
  if (lane_swap) {
    os << ",\"lane_swap_crossed\":" << (st.lane_swap_cross ? "true" : "false") << ",\"measure_records_swap\":[";
    for (int j = 0; j < st.T; ++j) {
      const ZregRecord r = zreg_record(st.zreg_swap[j]);
      os << (j ? "," : "") << "[" << r.wht << "," << r.lane << "," << r.wave << "," << r.neg << "]";
    }
    os << "],\"measure_swap_bits\":[";
    for (int i = 0; i < 4; ++i) os << (i ? "," : "") << (int)st.zreg_swap_bits[i];
    os << "],\"measure_swap_thread_bits\":[";
    for (int t = 0; t < st.T - 4; ++t) os << (t ? "," : "") << (int)st.zreg_swap_thread_bits[t];
    os << "],\"measure_between\":[";
    for (size_t i = 0; i + 1 < st.zreg_between.size(); i += 2)
      os << (i ? "," : "") << "[" << (int)st.zreg_between[i] << "," << (int)st.zreg_between[i + 1] << "]";
    os << "]";
  }
  if (from_regs) {
    os << ",\"measure_records\":[";
    for (int j = 0; j < st.T; ++j) {
      const ZregRecord r = zreg_record(st.zreg[j]);
      os << (j ? "," : "") << "[" << r.wht << "," << r.lane << "," << r.wave << "," << r.neg << "]";
    }
    os << "],\"measure_group_bits\":[";
    for (int i = 0; i < 4; ++i) os << (i ? "," : "") << (int)st.zreg_bits[i];
    os << "],\"measure_thread_bits\":[";
    for (int t = 0; t < st.T - 4; ++t) os << (t ? "," : "") << (int)st.zreg_thread_bits[t];
    os << "],\"measure_after\":[";
    for (size_t i = 0; i + 1 < st.zreg_after.size(); i += 2)
      os << (i ? "," : "") << "[" << (int)st.zreg_after[i] << "," << (int)st.zreg_after[i + 1] << "]";
    os << "]";
  }
}

std::string describe_plan(const qmle_plan *p) {
  std::ostringstream os;
  os << "{\"n_qubits\":" << p->n << ",\"n_ops\":" << p->ops.size()
     << ",\"n_lowered\":" << p->lowered.size()
     << ",\"whole_state_lds\":" << (p->whole_state_lds ? "true" : "false")
     << ",\"model_cost\":" << p->model_cost << ",\"candidate\":" << p->chosen_candidate
     << ",\"autotuned\":" << (p->autotuned ? "true" : "false")
     << ",\"zero_run\":" << ((p->flags & QMLE_PLAN_INTERNAL_ZERO_RUN) ? "true" : "false") << ",\"tile_bits\":" << p->tile_T << ",\"low_bits\":" << p->tile_L
     << ",\"mat_floats\":" << p->mat_floats_unit << ",\"mat_floats_old\":" << p->mat_floats_old
     << ",\"mat_row_floats\":" << p->mat_floats
     << ",\"build_groups\":" << p->groups.size() << ",\"build_groups_needed\":" << p->n_groups_needed
     << ",\"algo_bytes_per_state\":" << p->algo_bytes_per_state
     << ",\"flops_per_state\":" << plan_flops_per_state(p) << ",\"stages\":[";
  for (size_t s = 0; s < p->stages.size(); ++s) {
    const Stage &st = p->stages[s];
    if (s) os << ",";
    os << "{\"kind\":\""
       << (st.kind == ST_DIRECT ? "direct" : st.kind == ST_TILE ? "tile" : "diag_all")
       << "\",\"n_lowered\":" << (st.op_end - st.op_begin) << ",\"T\":" << st.T
       << ",\"L\":" << st.L << ",\"shift\":" << st.shift << ",\"lds_round_trips\":" << (st.grp_end - st.grp_begin)
       << ",\"algo_bytes_per_state\":"
       << st.algo_bytes_per_state + (s + 1 == p->stages.size() ? p->extra_algo_last_stage : 0.0)
       << ",\"flops_per_state\":" << stage_flops_per_state(p, st, false)
       << ",\"flops_live_per_state\":" << stage_flops_per_state(p, st, true)
       << ",\"zero_in\":" << st.zero_in << ",\"next_tile\":" << (st.next_tile ? "true" : "false")
       << ",\"product\":" << (st.product_ok ? "true" : "false") << ",\"expval_kernel\":\""
       << kTileFamilyNames[expval_kernel_of(p, s, !(p->flags & QMLE_PLAN_NO_SPARSE))]
       << "\",\"read_bytes_from_zero\":" << (unsigned long long)stage_read_bytes(p, s)
       << ",\"write_bytes_from_zero\":" << (unsigned long long)stage_write_bytes(p, s)
       << ",\"bits\":[";
    for (int i = 0; i < st.T; ++i) os << (i ? "," : "") << (int)st.tile_bits[i];
    os << "],\"groups\":[";
    for (int g = st.grp_begin; g < st.grp_end; ++g) {
      const OpGroup &og = p->op_groups[g];
      os << (g > st.grp_begin ? "," : "") << "{\"kind\":" << (int)og.kind << ",\"n_ops\":"
         << (int)og.n_ops << ",\"bits\":[" << (int)og.bits[0] << "," << (int)og.bits[1] << ","
         << (int)og.bits[2] << "," << (int)og.bits[3] << "]}";
    }
    os << "],\"fast\":" << (st.fast_ok ? "true" : "false") << ",\"fast_groups\":[";
    for (int g = st.fast_begin; g < st.fast_end; ++g) {
      os << (g > st.fast_begin ? "," : "") << "{\"n_ops\":" << p->groups2[g].n_ops
         << ",\"relayout\":" << (int)p->groups2[g].relayout
         << ",\"sync_before\":" << ((p->groups2[g].sync & 1) ? "true" : "false");
      // what the group's tables were emitted from: slot of amplitude c of work item t = sw(XOR of the columns of
      // e(t, c) ^ const), thread bit k of t at position thread_bits[k], bit i of c at position bits[i]
      const Stage::FastGroupInfo &fi = st.fast_info[g - st.fast_begin];
      os << ",\"bits\":[";
      for (int i = 0; i < 4; ++i) os << (i ? "," : "") << (int)fi.bits[i];
      os << "],\"thread_bits\":[";
      for (int t = 0; t < st.T - 4; ++t) os << (t ? "," : "") << (int)fi.thread_bits[t];
      os << "],\"layout_cols\":[";
      for (int j = 0; j < st.T; ++j) os << (j ? "," : "") << fi.cols[j];
      os << "],\"layout_const\":" << fi.cnst << "}";
    }
    os << "]";
    describe_measuring(os, p, s);
    if (st.kind == ST_TILE) {
      // ops of the stage's fast stream (concatenated fast_groups) that run in unit-pivot form, and the carriers that
      // take their chains' pivots (assign_unit_forms); fast_ops: each op's dispatch code and matrix-row offset
      os << ",\"unit_form_ops\":[";
      for (size_t i = 0; i < st.unit_form_ops.size(); ++i) os << (i ? "," : "") << st.unit_form_ops[i];
      os << "],\"scale_carriers\":[";
      for (size_t i = 0; i < st.scale_carriers.size(); ++i) os << (i ? "," : "") << st.scale_carriers[i];
      os << "],\"fast_ops\":[";
      if (st.fast_ok && st.fast_end > st.fast_begin) {
        uint32_t k = p->groups2[st.fast_begin].op_begin;
        bool any = false;
        for (int g = st.fast_begin; g < st.fast_end; ++g)
          for (int j = 0; j < (int)p->groups2[g].n_ops; ++j, ++k, any = true)
            os << (any ? "," : "") << "[" << (int)p->ops2[k].pad << "," << p->ops2[k].mat_off << "]";
      }
      // per fast group (the entries of "fast_groups" stay what they were): whether it runs in product form
      // (assign_product_forms) and the float offset of its record in the matrix row (-1: none)
      os << "],\"product_form_groups\":[";
      for (int g = st.fast_begin; g < st.fast_end; ++g)
        os << (g > st.fast_begin ? "," : "") << ((p->groups2[g].sync & kGroupProduct) ? "true" : "false");
      os << "],\"product_form_records\":[";
      for (int g = st.fast_begin; g < st.fast_end; ++g)
        os << (g > st.fast_begin ? "," : "") << ((p->groups2[g].sync & kGroupProduct) ? (long long)p->groups2[g].prod_off : -1ll);
      // ... and whether a run that ends this stage in |amplitude|^2 may build that record without a closing diagonal
      // (mark_closing_free_groups); measured_form_last_run: the last batch run did, for its last stage, and ran them
      os << "],\"closing_free_groups\":[";
      for (int g = st.fast_begin; g < st.fast_end; ++g)
        os << (g > st.fast_begin ? "," : "") << ((p->groups2[g].sync & kGroupClosingFree) ? "true" : "false");
      os << "],\"group_product_form_last_run\":" << (s < 64 && ((p->last_run.product_form_stages >> s) & 1u) ? "true" : "false")
         << ",\"measured_form_last_run\":" << (s + 1 == p->stages.size() && p->last_run.measured_form ? "true" : "false");
    }
    if (s + 1 == p->stages.size())
      os << ",\"measure_tiles_per_workgroup_last_run\":" << p->last_run.measure_tpw
         << ",\"measured_from_registers_last_run\":" << (p->last_run.measure_regs ? "true" : "false")
         << ",\"wave_private_walk_last_run\":" << (p->last_run.wave_private ? "true" : "false")
         << ",\"staging_dma_last_run\":" << (p->last_run.staging_dma ? "true" : "false")
         << ",\"last_group_lane_swap_last_run\":" << (p->last_run.lane_swap ? "true" : "false")
         << ",\"chunk_loop_last_run\":\"" << kChunkLoopNames[p->last_run.chunk_loop] << "\""
         << ",\"matrices_from_map_last_run\":" << (p->last_run.matrices_from_map ? "true" : "false")
         << ",\"walk_kernel_last_run\":" << (p->last_run.walk_kernel ? "true" : "false")
         << ",\"mw_finish_last_run\":\"" << kMwFinishNames[p->last_run.mw_finish] << "\"";
    os << ",\"src_ops\":[";
    for (size_t i = 0; i < st.src_ops.size(); ++i) os << (i ? "," : "") << st.src_ops[i];
    os << "]}";
  }
  os << "]";
  if (p->expval_child)
    os << ",\"absorbed_ops\":" << p->absorbed.size()
       << ",\"expval_plan\":" << describe_plan(p->expval_child);
  os << "}";
  return os.str();
}

}  // namespace qmle
