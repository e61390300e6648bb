// nlj.hip — NestedLoopJoinExec / CrossJoinExec (joins/nested_loop_join.rs, joins/cross_join.rs): joins without an equality key.
//
// The predicate is evaluated over the pair space itself: k_nlj gives every lane one right (probe) row, stages the left (build) rows
// through LDS a tile at a time and runs the filter's row program (rowprog.hpp) once per pair, entirely in registers.  Only pairs that
// pass are written, and the six one-sided join types write no pair at all.  Filters the row-program compiler declines (division,
// LIKE, Utf8 columns, too many columns / registers / instructions) and joins without a filter take the materialising path in bounded
// pieces of the pair space (k_nlj_cartesian + the column-at-a-time evaluator).  Both end in the tail the filtered hash join has:
// passing pairs, right hit bytes and left visited bytes -> the join type's table (join.hip's pieces behind internal.hpp).
//
// Output order (include/dfgpu.h): passing pairs in right-row-major order, then the unmatched right rows, then the
// unmatched left rows; the one-sided types in their side's row order.
//
// Below it, sharing the tail: the range join (dfgpu_range_join) — range conditions on one right column by sorting that
// column and searching the bounds, without the pair space.
#include "internal.hpp"
#include "rowprog_host.hpp"

namespace dfgpu {

constexpr int NLJ_TL = BLOCK;  // left rows per LDS tile: one staged row per lane
enum NljMode : int { NLJ_FLAGS = 0, NLJ_COUNT = 1, NLJ_EMIT = 2 };

struct NljArgs {
  RowProgram p;
  int n_prologue, n_pred_end, pred_reg;
  uint32_t left_regs;              // bit c = column slot c (= register c) is read from the left table
  int n_left;
  uint8_t left_slot[RP_MAX_COLS];  // the left table's slots, in slot order
  int64_t nl, nr, chunk_rows;
  int n_chunks;
  int early_exit;                  // FLAGS: nothing reads the left visited bytes, a wave stops once all its rows matched
  uint8_t* hit;                    // [nr] right row has a passing pair (zeroed by the host), or null
  uint8_t* visited;                // [nl] left row has a passing pair (zeroed by the host), or null
  uint32_t* counts;                // COUNT: [nr * n_chunks] passing pairs of (right row, chunk)
  const uint64_t* offsets;         // EMIT: exclusive prefix of counts (nr * n_chunks + 1 entries)
  int64_t* out_l;
  int64_t* out_r;
};

// column slot c of `row`, widened to the register form (rp_load_row's rules)
__device__ __forceinline__ void nlj_load(const RowProgram& p, int c, int64_t row, uint64_t& lo, uint64_t& hi, bool& isnull) {
  const void* d = p.col_data[c];
  lo = 0;
  hi = 0;
  switch (p.col_kind[c]) {
    case RPL_I32: lo = (uint64_t)(int64_t)((const int32_t*)d)[row]; hi = (uint64_t)((int64_t)lo >> 63); break;
    case RPL_U32: lo = ((const uint32_t*)d)[row]; break;
    case RPL_I64: lo = ((const uint64_t*)d)[row]; hi = (uint64_t)((int64_t)lo >> 63); break;
    case RPL_U64: case RPL_F64: lo = ((const uint64_t*)d)[row]; break;
    case RPL_U8: lo = ((const uint8_t*)d)[row]; break;
    case RPL_I128: { const uint64_t* q = (const uint64_t*)d + 2 * row; lo = q[0]; hi = q[1]; break; }
    default: lo = (((const uint64_t*)d)[row >> 6] >> (row & 63)) & 1ull; break;  // RPL_BOOL
  }
  const uint64_t* v = p.col_valid[c];
  isnull = v ? !bit_at(v, row) : false;
}

// grid: x = blocks of blockDim.x right rows (one per lane), y = chunks of `chunk_rows` left rows.  blockDim.x is BLOCK, or fewer
// whole waves when the right side is shorter than that (a lane without a right row would walk every tile for nothing).  LDS: lo / hi
// of every left slot for NLJ_TL rows, then one word of NULL bits per row.
template <int NREG, int MODE>
__global__ __launch_bounds__(BLOCK) void k_nlj(const NljArgs a) {
  extern __shared__ uint64_t nlj_lds[];
  uint64_t* s_lo = nlj_lds;
  uint64_t* s_hi = nlj_lds + (size_t)a.n_left * NLJ_TL;
  uint32_t* s_nulls = reinterpret_cast<uint32_t*>(nlj_lds + (size_t)2 * a.n_left * NLJ_TL);

  const int64_t rrow = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = rrow < a.nr;
  const int chunk = (int)blockIdx.y;
  const int64_t l0 = (int64_t)chunk * a.chunk_rows;
  const int64_t l1 = l0 + a.chunk_rows < a.nl ? l0 + a.chunk_rows : a.nl;

  RP_DECLARE_REGS(r, NREG);
  rp_exec(a.p, 0, a.n_prologue, r);
  if (active) {
    uint32_t nulls = r.nulls;
#pragma unroll
    for (int c = 0; c < RP_MAX_COLS; c++) {
      if (c < a.p.n_cols && !((a.left_regs >> c) & 1u)) {
        uint64_t lo, hi;
        bool isnull;
        nlj_load(a.p, c, rrow, lo, hi, isnull);
        r.set(c, lo, hi);
        nulls = (nulls & ~(1u << c)) | ((isnull ? 1u : 0u) << c);
      }
    }
    r.nulls = nulls;
  }

  bool matched = false;
  uint32_t cnt = 0;
  int64_t pos = 0, pos_end = 0;
  if (MODE == NLJ_EMIT && active) {
    pos = (int64_t)a.offsets[rrow * a.n_chunks + chunk];
    pos_end = (int64_t)a.offsets[rrow * a.n_chunks + chunk + 1];
  }

  for (int64_t base = l0; base < l1; base += NLJ_TL) {
    const int tile = (int)(l1 - base < NLJ_TL ? l1 - base : NLJ_TL);
    // ---- stage: a lane widens left row base + i (coalesced loads; one LDS row per lane in a full workgroup)
    for (int i = (int)threadIdx.x; i < tile; i += (int)blockDim.x) {
      uint32_t nb = 0;
      for (int j = 0; j < a.n_left; j++) {
        const int c = a.left_slot[j];
        uint64_t lo, hi;
        bool isnull;
        nlj_load(a.p, c, base + i, lo, hi, isnull);
        s_lo[j * NLJ_TL + i] = lo;
        s_hi[j * NLJ_TL + i] = hi;
        nb |= (isnull ? 1u : 0u) << c;
      }
      s_nulls[i] = nb;
    }
    __syncthreads();
    // ---- walk: every lane evaluates its right row against left row base + t (LDS reads at a wave-uniform address: broadcasts)
    const bool wave_done = MODE == NLJ_FLAGS && a.early_exit && __all(matched || !active);
    if (!wave_done) {
      for (int t = 0; t < tile; t++) {
        for (int j = 0; j < a.n_left; j++) r.set(a.left_slot[j], s_lo[j * NLJ_TL + t], s_hi[j * NLJ_TL + t]);
        r.nulls = (r.nulls & ~a.left_regs) | s_nulls[t];
        rp_exec(a.p, a.n_prologue, a.n_pred_end, r);
        const bool pass = active && rp_true(r, a.pred_reg);
        if (MODE == NLJ_EMIT) {
          if (pass && pos < pos_end) {
            a.out_l[pos] = base + t;
            a.out_r[pos] = rrow;
            pos++;
          }
        } else {
          if (pass) {
            matched = true;
            cnt++;
          }
          if (a.visited) {
            const uint64_t any = ballot64(pass);  // one store per wave and left row; storing 1 twice is harmless
            if (any && lane_id() == (unsigned)__builtin_ctzll(any)) a.visited[base + t] = 1;
          } else if (MODE == NLJ_FLAGS && a.early_exit) {
            if (__all(matched || !active)) break;
          }
        }
      }
    }
    // the tile is reused by the next stage; a workgroup whose right rows have all matched has nothing left to learn
    if (MODE == NLJ_FLAGS && a.early_exit) {
      if (__syncthreads_and(matched || !active)) break;
    } else {
      __syncthreads();
    }
  }
  if (MODE != NLJ_EMIT && active) {
    if (MODE == NLJ_COUNT) a.counts[rrow * a.n_chunks + chunk] = cnt;
    if (a.hit && matched) a.hit[rrow] = 1;
  }
}

// pair j of the pair space in right-row-major order: (left j % nl, right j / nl), for j in [j0, j0 + m)
__global__ __launch_bounds__(BLOCK) void k_nlj_cartesian(int64_t j0, int64_t m, int64_t nl, int64_t* __restrict__ out_l, int64_t* __restrict__ out_r) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * BLOCK) {
    const int64_t j = j0 + i, rr = j / nl;
    out_l[i] = j - rr * nl;
    out_r[i] = rr;
  }
}
// hit / visited bytes of the passing pairs (bytes zeroed by the host; storing 1 twice is harmless)
__global__ __launch_bounds__(BLOCK) void k_nlj_mark(const int64_t* __restrict__ pl, const int64_t* __restrict__ pr, const uint64_t* __restrict__ pass, int64_t m,
                                                   uint8_t* __restrict__ hit, uint8_t* __restrict__ visited) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * BLOCK) {
    if (!bit_at(pass, i)) continue;
    hit[pr[i]] = 1;
    visited[pl[i]] = 1;
  }
}

namespace {

bool pairs_out(int jt) { return jt == DFGPU_JOIN_INNER || jt == DFGPU_JOIN_LEFT || jt == DFGPU_JOIN_RIGHT || jt == DFGPU_JOIN_FULL; }
bool right_one_sided(int jt) { return jt == DFGPU_JOIN_RIGHT_SEMI || jt == DFGPU_JOIN_RIGHT_ANTI || jt == DFGPU_JOIN_RIGHT_MARK; }

int64_t out_row_bytes(const Table& t, const std::vector<int>& cols) {
  int64_t b = 0;
  for (int c : cols) b += t.cols[c].field.type == DFGPU_UTF8 ? 8 : t.cols[c].field.type == DFGPU_BOOL ? 1 : type_width(t.cols[c].field.type);
  return b;
}

// what both evaluations hand to the tail
struct NljMatches {
  BufPtr hit, visited;      // bytes per right / left row (64 bytes of padding)
  BufPtr pl, pr;            // pair types: passing pairs in right-row-major order, with room for the unmatched rows behind them
};

// passing pairs + hit bytes + visited bytes -> the join type's table (adjust_indices_by_join_type, joins/utils.rs:1432-1488, and
// process_unmatched_build_batch in one call).  `fill_pairs(left ids, right ids)` is called once the output is counted, admitted and
// allocated: it writes the n_pass passing pairs to the front of the buffers; the unmatched rows are appended behind them here.
template <class F>
Table nlj_tail(const Table& left, const Table& right, int jt, const std::vector<int>& lout, const std::vector<int>& rout, NljMatches& M, int64_t n_pass,
               F&& fill_pairs) {
  Runtime& r = rt();
  const int64_t nl = left.nrows, nr = right.nrows;
  Table out;
  out.device = left.device;
  if (pairs_out(jt)) {
    const bool right_outer = jt == DFGPU_JOIN_RIGHT || jt == DFGPU_JOIN_FULL, left_outer = jt == DFGPU_JOIN_LEFT || jt == DFGPU_JOIN_FULL;
    BufPtr rmask, rprefix, lmask, lprefix;
    int64_t n_ur = 0, n_ul = 0;
    if (right_outer && nr) {
      const int64_t nw = (nr + 63) / 64;
      rmask = make_buf(bitmap_bytes(nr));
      rprefix = make_buf((size_t)(nw + 1) * 8);
      join_bytes_mask(M.hit->as<uint8_t>(), nr, false, rmask->as<uint64_t>());
      scan_mask_popcounts(rmask->as<uint64_t>(), nullptr, nr, rprefix->as<uint64_t>());
      n_ur = (int64_t)read_u64(rprefix->as<uint64_t>() + nw);
    }
    if (left_outer && nl) {
      const int64_t nw = (nl + 63) / 64;
      lmask = make_buf(bitmap_bytes(nl));
      lprefix = make_buf((size_t)(nw + 1) * 8);
      join_bytes_mask(M.visited->as<uint8_t>(), nl, false, lmask->as<uint64_t>());
      scan_mask_popcounts(lmask->as<uint64_t>(), nullptr, nl, lprefix->as<uint64_t>());
      n_ul = (int64_t)read_u64(lprefix->as<uint64_t>() + nw);
    }
    const int64_t n_out = n_pass + n_ur + n_ul;
    // the counted output is admitted before a pair is written: 16 bytes of row ids and the output columns per row
    pool_admit(n_out * (16 + out_row_bytes(left, lout) + out_row_bytes(right, rout)));
    M.pl = make_buf((size_t)(n_out ? n_out : 1) * 8);
    M.pr = make_buf((size_t)(n_out ? n_out : 1) * 8);
    fill_pairs(M.pl->as<int64_t>(), M.pr->as<int64_t>());
    if (n_ur) join_append_unmatched(rmask->as<uint64_t>(), rprefix->as<uint64_t>(), nr, n_pass, M.pl->as<int64_t>(), M.pr->as<int64_t>());
    if (n_ul) join_append_unmatched(lmask->as<uint64_t>(), lprefix->as<uint64_t>(), nl, n_pass + n_ur, M.pr->as<int64_t>(), M.pl->as<int64_t>());
    out.nrows = n_out;
    for (Column& c : gather_columns(left, lout, M.pl->as<int64_t>(), n_out, right_outer)) out.cols.push_back(std::move(c));
    for (Column& c : gather_columns(right, rout, M.pr->as<int64_t>(), n_out, left_outer)) out.cols.push_back(std::move(c));
  } else {
    const bool rs = right_one_sided(jt);
    const Table& side = rs ? right : left;
    const std::vector<int>& cols = rs ? rout : lout;
    const uint8_t* bytes = (rs ? M.hit : M.visited)->as<uint8_t>();
    const int64_t n = side.nrows;
    if (jt == DFGPU_JOIN_LEFT_MARK || jt == DFGPU_JOIN_RIGHT_MARK) {
      out.nrows = n;
      for (int c : cols) out.cols.push_back(side.cols[c]);
      out.cols.push_back(mark_column(bytes, n));
    } else {
      BufPtr mask = make_zero_buf(bitmap_bytes(n ? n : 1));
      join_bytes_mask(bytes, n, jt == DFGPU_JOIN_LEFT_SEMI || jt == DFGPU_JOIN_RIGHT_SEMI, mask->as<uint64_t>());
      out = compact_table(side, cols, mask->as<uint64_t>(), nullptr);
    }
  }
  DFGPU_HIP(hipStreamSynchronize(r.stream));
  return out;
}

// ---- the row-program path
struct NljPlan {
  NljArgs a{};
  int n_regs = 0;
  int64_t filter_row_bytes_l = 0, filter_row_bytes_r = 0;
};

// lanes of a workgroup: BLOCK, or the whole waves a shorter right side fills
int nlj_block(int64_t nr) { return nr >= BLOCK ? BLOCK : (int)std::max<int64_t>(WAVE, (nr + WAVE - 1) / WAVE * WAVE); }

template <int MODE>
void launch_nlj(const NljPlan& P, const NljArgs& a) {
  const int block = nlj_block(a.nr);
  const dim3 grid((unsigned)((a.nr + block - 1) / block), (unsigned)a.n_chunks);
  const size_t lds = (size_t)a.n_left * NLJ_TL * 16 + (size_t)NLJ_TL * 4;
  auto kern = P.n_regs <= 16 ? k_nlj<16, MODE> : k_nlj<32, MODE>;
  kern<<<grid, block, lds, rt().stream>>>(a);
  DFGPU_HIP(hipGetLastError());
}

Table nlj_rowprog(const Table& left, const Table& right, int jt, const std::vector<int>& lout, const std::vector<int>& rout, NljPlan& P) {
  const int64_t nl = left.nrows, nr = right.nrows;
  NljArgs& a = P.a;
  a.nl = nl;
  a.nr = nr;
  // chunks of left rows: four waves per SIMD (what the kernel's registers allow) even when the right side is short, while the count
  // array (4 bytes per right row and chunk) stays within the rows worth a pass
  const int block = nlj_block(nr);
  const int64_t nbx = (nr + block - 1) / block;
  int64_t chunk_rows = option_int("nlj.left_chunk_rows", 0);
  if (chunk_rows <= 0) {
    const int64_t waves = (int64_t)policy().num_cus * 16, per_chunk = nbx * (block / WAVE);
    int64_t want = per_chunk ? (waves + per_chunk - 1) / per_chunk : 1;
    if (nr) want = std::min<int64_t>(want, std::max<int64_t>(1, policy().rows_worth_a_pass() / nr));
    want = std::max<int64_t>(1, std::min<int64_t>(want, (nl + NLJ_TL - 1) / NLJ_TL));
    chunk_rows = ((nl + want - 1) / want + NLJ_TL - 1) / NLJ_TL * NLJ_TL;
  }
  if (chunk_rows < 1) chunk_rows = 1;
  const int64_t n_chunks = std::max<int64_t>(1, (nl + chunk_rows - 1) / chunk_rows);
  DFGPU_CHECK(n_chunks <= 65535, "nlj.left_chunk_rows gives more than 65535 chunks of left rows");
  DFGPU_CHECK(nr * n_chunks < (int64_t)1 << 40, "nested loop join: the right side is too long for the pair count pass");
  a.chunk_rows = chunk_rows;
  a.n_chunks = (int)n_chunks;

  NljMatches M;
  M.hit = make_zero_buf((size_t)nr + 64);
  M.visited = make_zero_buf((size_t)nl + 64);
  const int64_t in_bytes = nl * P.filter_row_bytes_l + nr * P.filter_row_bytes_r;
  if (!pairs_out(jt)) {
    const bool rs = right_one_sided(jt);
    a.hit = rs ? M.hit->as<uint8_t>() : nullptr;
    a.visited = rs ? nullptr : M.visited->as<uint8_t>();
    a.early_exit = rs && option_on("nlj.early_exit", true);
    if (nr) {
      ProfileScope ps("nlj_flags", in_bytes + (rs ? nr : nl));
      launch_nlj<NLJ_FLAGS>(P, a);
    }
    return nlj_tail(left, right, jt, lout, rout, M, 0, [](int64_t*, int64_t*) {});
  }
  a.hit = (jt == DFGPU_JOIN_RIGHT || jt == DFGPU_JOIN_FULL) ? M.hit->as<uint8_t>() : nullptr;
  a.visited = (jt == DFGPU_JOIN_LEFT || jt == DFGPU_JOIN_FULL) ? M.visited->as<uint8_t>() : nullptr;
  const int64_t n_counts = nr * n_chunks;
  BufPtr counts = make_buf((size_t)(n_counts ? n_counts : 1) * 4), offsets = make_zero_buf((size_t)(n_counts + 1) * 8);
  int64_t n_pass = 0;
  if (nr) {
    a.counts = counts->as<uint32_t>();
    {
      ProfileScope ps("nlj_count", in_bytes + n_counts * 4 + (a.hit ? nr : 0) + (a.visited ? nl : 0));
      launch_nlj<NLJ_COUNT>(P, a);
    }
    scan_u32(counts->as<uint32_t>(), n_counts, offsets->as<uint64_t>());
    n_pass = (int64_t)read_u64(offsets->as<uint64_t>() + n_counts);
  }
  return nlj_tail(left, right, jt, lout, rout, M, n_pass, [&](int64_t* pl, int64_t* pr) {
    if (!n_pass) return;
    NljArgs e = a;
    e.hit = nullptr;
    e.visited = nullptr;
    e.counts = nullptr;
    e.offsets = offsets->as<uint64_t>();
    e.out_l = pl;
    e.out_r = pr;
    ProfileScope ps("nlj_emit", in_bytes + n_counts * 8 + n_pass * 16);
    launch_nlj<NLJ_EMIT>(P, e);
  });
}

// ---- the materialising path: pieces of the pair space -> intermediate batch -> expression -> pass mask
Table nlj_materialised(const Table& left, const Table& right, int jt, const dfgpu_join_filter* jf, const std::vector<int>& lout, const std::vector<int>& rout) {
  Runtime& r = rt();
  const int64_t nl = left.nrows, nr = right.nrows;
  DFGPU_CHECK(nl == 0 || nr <= INT64_MAX / 32 / nl, "nested loop join: the pair space does not fit 64 bits");
  const int64_t total = nl * nr;
  const bool want_pairs = pairs_out(jt);
  // a piece holds 16 bytes of row ids per pair, the gathered intermediate columns, and the expression's temporaries (taken as
  // as much again): a quarter of what the pool may still hand out, so that the kept pairs and the output have room beside it
  int64_t per_pair = 16 + 1;
  if (jf)
    for (int i = 0; i < jf->n_columns; i++) {
      const Column& c = (jf->column_side[i] == 0 ? left : right).cols[jf->column_index[i]];
      per_pair += 2 * (c.field.type == DFGPU_UTF8 ? 32 : c.field.type == DFGPU_BOOL ? 1 : type_width(c.field.type));
    }
  int64_t chunk_pairs = option_int("nlj.chunk_pairs", 0);
  if (chunk_pairs <= 0) chunk_pairs = std::max<int64_t>(1 << 16, std::min<int64_t>((int64_t)1 << 28, pool_free_bytes() / 4 / per_pair));
  if (!jf && want_pairs) pool_admit(total * (16 + out_row_bytes(left, lout) + out_row_bytes(right, rout)));  // a cross join's size is known

  NljMatches M;
  M.hit = make_zero_buf((size_t)nr + 64);
  M.visited = make_zero_buf((size_t)nl + 64);
  struct Piece { BufPtr l, r; int64_t n; };
  std::vector<Piece> kept;
  int64_t n_pass = 0;
  for (int64_t j0 = 0; j0 < total; j0 += chunk_pairs) {
    const int64_t m = std::min(chunk_pairs, total - j0), m_words = (m + 63) / 64;
    BufPtr pl = make_buf((size_t)m * 8), pr = make_buf((size_t)m * 8);
    {
      ProfileScope ps("nlj_cartesian", m * 16);
      k_nlj_cartesian<<<grid_for(m, BLOCK), BLOCK, 0, r.stream>>>(j0, m, nl, pl->as<int64_t>(), pr->as<int64_t>());
      DFGPU_HIP(hipGetLastError());
    }
    BufPtr pass = make_buf((size_t)m_words * 8);
    DFGPU_HIP(hipMemsetAsync(pass->ptr, jf ? 0 : 0xFF, (size_t)m_words * 8, r.stream));
    if (jf) {
      Table inter;
      inter.nrows = m;
      for (int i = 0; i < jf->n_columns; i++) {
        const bool is_left = jf->column_side[i] == 0;
        inter.cols.push_back(gather_column((is_left ? left : right).cols[jf->column_index[i]], (is_left ? pl : pr)->as<int64_t>(), m, false));
      }
      Datum d = evaluate(jf->expression, inter);
      DFGPU_CHECK(d.col.field.type == DFGPU_BOOL, "join filter expression must be Boolean");
      Column mc = datum_to_column(d, m, "");
      if (mc.validity) and_bitmaps(mc.data->as<uint64_t>(), mc.valid_words(), m_words, pass->as<uint64_t>());
      else pass = mc.data;
    }
    k_nlj_mark<<<grid_for(m, BLOCK), BLOCK, 0, r.stream>>>(pl->as<int64_t>(), pr->as<int64_t>(), pass->as<uint64_t>(), m, M.hit->as<uint8_t>(), M.visited->as<uint8_t>());
    DFGPU_HIP(hipGetLastError());
    if (want_pairs) {
      BufPtr prefix = make_buf((size_t)(m_words + 1) * 8);
      scan_mask_popcounts(pass->as<uint64_t>(), nullptr, m, prefix->as<uint64_t>());
      const int64_t k = (int64_t)read_u64(prefix->as<uint64_t>() + m_words);
      if (k) {
        pool_admit((n_pass + k) * 16);
        Piece pc{make_buf((size_t)k * 8), make_buf((size_t)k * 8), k};
        join_pairs_compact(pl->as<int64_t>(), pr->as<int64_t>(), pass->as<uint64_t>(), prefix->as<uint64_t>(), m, pc.l->as<int64_t>(), pc.r->as<int64_t>());
        kept.push_back(std::move(pc));
        n_pass += k;
      }
    }
  }
  return nlj_tail(left, right, jt, lout, rout, M, n_pass, [&](int64_t* pl, int64_t* pr) {
    int64_t at = 0;
    for (const Piece& pc : kept) {
      DFGPU_HIP(hipMemcpyAsync(pl + at, pc.l->ptr, (size_t)pc.n * 8, hipMemcpyDeviceToDevice, r.stream));
      DFGPU_HIP(hipMemcpyAsync(pr + at, pc.r->ptr, (size_t)pc.n * 8, hipMemcpyDeviceToDevice, r.stream));
      at += pc.n;
    }
  });
}

// the filter as a predicate-only row program over a zero-copy view of its columns; false = the compiler declined it
bool nlj_compile(const Table& view, const dfgpu_join_filter& jf, NljPlan& P) {
  CompiledProgram cp;
  std::vector<int> slot_cols;
  try {
    RowProgramCompiler comp(view);
    comp.set_predicate(jf.expression);
    std::string why;
    if (!comp.finish(cp, why)) {
      if (trace_on("join")) fprintf(stderr, "[nlj] row program declined: %s\n", why.c_str());
      return false;
    }
    slot_cols = comp.slot_columns();
  } catch (const Error&) {
    return false;  // lowering went on past a declined node and met an operand it cannot type: the evaluator decides
  }
  if (cp.pred_reg < 0) return false;
  NljArgs& a = P.a;
  a.p = cp.prog;
  a.n_prologue = cp.n_prologue;
  a.n_pred_end = cp.n_pred_end;
  a.pred_reg = cp.pred_reg;
  P.n_regs = cp.n_regs;
  for (int s = 0; s < (int)slot_cols.size(); s++) {
    const Column& c = view.cols[slot_cols[s]];
    const int64_t w = c.field.type == DFGPU_BOOL ? 1 : type_width(c.field.type);
    if (jf.column_side[slot_cols[s]] == 0) {
      a.left_regs |= 1u << s;
      a.left_slot[a.n_left++] = (uint8_t)s;
      P.filter_row_bytes_l += w;
    } else {
      P.filter_row_bytes_r += w;
    }
  }
  return true;
}

}  // namespace

Table nested_loop_join(const Table& left, const Table& right, int jt, const dfgpu_join_filter* jf, const std::vector<int>& lout, const std::vector<int>& rout) {
  DFGPU_CHECK(left.device == right.device, "the right table lives on another device than the left table (move it with dfgpu_table_copy_to_device)");
  for (int c : lout) DFGPU_CHECK(c >= 0 && c < (int)left.cols.size(), "left output column out of range");
  for (int c : rout) DFGPU_CHECK(c >= 0 && c < (int)right.cols.size(), "right output column out of range");
  if (jf) {
    Table view;
    view.device = left.device;
    std::shared_ptr<const DictValues> dict;
    for (int i = 0; i < jf->n_columns; i++) {
      DFGPU_CHECK(jf->column_side[i] == 0 || jf->column_side[i] == 1, "join filter column side must be 0 (left) or 1 (right)");
      const Table& side = jf->column_side[i] == 0 ? left : right;
      DFGPU_CHECK(jf->column_index[i] >= 0 && jf->column_index[i] < (int)side.cols.size(), "join filter column index out of range");
      view.cols.push_back(side.cols[jf->column_index[i]]);
      if (view.cols.back().dict) {
        // dictionary codes are compared as integers: that is only the strings' comparison when the columns share their dictionary
        DFGPU_CHECK(!dict || same_dictionary(dict, view.cols.back().dict), "join filter over dictionary-encoded columns with different dictionaries: decode them first (dfgpu_table_dictionary_decode)");
        dict = view.cols.back().dict;
      }
    }
    DFGPU_CHECK(expr_type(jf->expression, view).type == DFGPU_BOOL, "join filter expression must be Boolean");
    NljPlan P;
    if (option_on("nlj.rowprog", true) && nlj_compile(view, *jf, P)) return nlj_rowprog(left, right, jt, lout, rout, P);
  }
  return nlj_materialised(left, right, jt, jf, lout, rout);
}

// ===================================================================================================================== range join
// dfgpu_range_join (ABI 20): `a <(=) x AND x <(=) b` over one right column x without the pair space.  The non-NULL x
// are sorted once as (orderable u64 key, row id) pairs; a left row's matches are then ONE run [lo, hi) of the sorted order, found by
// two binary searches (k_rj_bounds).  The right rows some run covers come from a difference array (+1 at lo, -1 at hi) and its scan
// (k_rj_cover) — no pair is enumerated for the six one-sided types and the unmatched tails.  The pair types expand the runs into
// (left row, right row) ids with the work split over OUTPUT SLOTS (k_rj_expand), and everything ends in nlj_tail above.
constexpr int RJ_TILE = DFGPU_RANGE_JOIN_TILE;
static_assert(RJ_TILE % BLOCK == 0 && RJ_TILE <= 65536, "a workgroup writes whole rounds of its lanes; tile-relative offsets are staged as u32");
// sorted keys every workgroup of k_rj_bounds stages in LDS: every stride-th key, so that the first 11 levels of each search are LDS
// reads.  16 KiB of the CU's 160 KiB: ten workgroups' staging fit, more than the eight 4-wave workgroups the 32-wave cap lets a CU hold,
// so the staging never lowers the occupancy.
constexpr int RJ_SAMPLES = 2048;
enum RjType : int { RJ_I32 = 0, RJ_U32 = 1, RJ_I64 = 2, RJ_U64 = 3, RJ_F64 = 4 };

// value i of a key column as a u64 whose unsigned order is the expression layer's order of the type: signed values sign-extended with
// bit 63 flipped; Float64 by the total order of its bits (negative: every bit flipped, else the sign bit)
template <int T>
__device__ __forceinline__ uint64_t rj_ordered(const void* d, int64_t i) {
  if (T == RJ_I32) return (uint64_t)(int64_t)((const int32_t*)d)[i] ^ (1ull << 63);
  if (T == RJ_U32) return ((const uint32_t*)d)[i];
  if (T == RJ_I64) return ((const uint64_t*)d)[i] ^ (1ull << 63);
  if (T == RJ_U64) return ((const uint64_t*)d)[i];
  const uint64_t b = ((const uint64_t*)d)[i];
  return b ^ ((uint64_t)((int64_t)b >> 63) | (1ull << 63));
}

// first position in [lo, hi) of the ascending `keys` whose key is >= q (UPPER: > q); hi when there is none
template <bool UPPER, class E, class Q>
__device__ __forceinline__ uint32_t rj_search(const E* keys, uint32_t lo, uint32_t hi, Q q) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const Q k = keys[mid];
    if (UPPER ? k <= q : k < q) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// the non-NULL rows of x, compacted in row order: key = ordered(x) - base, idx = the row (idx null: no NULLs, the position is the row)
template <int T>
__global__ __launch_bounds__(BLOCK) void k_rj_keys(const void* __restrict__ x, const uint64_t* __restrict__ valid, const uint64_t* __restrict__ prefix, int64_t n,
                                                   uint64_t base, uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) {
    int64_t pos = i;
    if (valid) {
      const uint64_t w = valid[i >> 6];
      if (!((w >> (i & 63)) & 1ull)) continue;
      pos = (int64_t)prefix[i >> 6] + __popcll(w & ((1ull << (i & 63)) - 1ull));
      idx[pos] = (uint32_t)i;
    }
    key[pos] = rj_ordered<T>(x, i) - base;
  }
}

struct RjBounds {
  const void* a;               // lower bound column (null: none) and its validity
  const uint64_t* a_valid;
  const void* b;               // upper bound column (null: none) and its validity
  const uint64_t* b_valid;
  int lower_inclusive, upper_inclusive;
  int64_t nl;
  const uint64_t* keys;        // [m] ascending: ordered(x) - base, every one <= span
  uint32_t m, stride, ns;      // the ns staged keys are keys[j * stride]
  uint64_t base, span;
  uint32_t* lo;                // [nl] start of the row's run in the sorted order
  uint32_t* count;             // [nl] its length
  uint8_t* visited;            // [nl] count != 0
  int32_t* diff;               // [m + 1] zeroed: +1 at lo, -1 at hi of every non-empty run; null when no right-side flag is needed
};

// position of left value `l` of `col` among the sorted keys: lower_bound, or upper_bound when `upper`
template <int T>
__device__ __forceinline__ uint32_t rj_position(const RjBounds& g, const uint64_t* s_keys, const void* col, int64_t l, bool upper) {
  const uint64_t v = rj_ordered<T>(col, l);
  if (v < g.base) return 0;
  const uint64_t q = v - g.base;
  if (q > g.span) return g.m;
  // staged keys before position j compare on q's near side, so the answer lies in ((j - 1) * stride, j * stride]
  const uint32_t j = upper ? rj_search<true>(s_keys, 0u, g.ns, q) : rj_search<false>(s_keys, 0u, g.ns, q);
  if (j == 0) return 0;
  const uint32_t lo = (j - 1) * g.stride + 1;
  const uint32_t hi = (uint64_t)j * g.stride < (uint64_t)g.m ? j * g.stride : g.m;
  return upper ? rj_search<true>(g.keys, lo, hi, q) : rj_search<false>(g.keys, lo, hi, q);
}

// one add per wave for the lanes that share the first adding lane's position (one x value matched by every left row would otherwise put
// every lane's atomic on one address), one per lane for the others.  Integer adds: the sums do not depend on arrival order.
__device__ __forceinline__ void rj_diff_add(int32_t* diff, bool on, uint32_t pos, int32_t delta) {
  const uint64_t adders = ballot64(on);
  if (!adders) return;
  const int leader = __builtin_ctzll(adders);
  const uint32_t lead_pos = (uint32_t)__shfl((int)pos, leader, 64);
  const uint64_t same = ballot64(on && pos == lead_pos);
  if ((int)lane_id() == leader) atomicAdd(diff + pos, delta * (int32_t)__popcll(same));
  else if (on && pos != lead_pos) atomicAdd(diff + pos, delta);
}

// one lane per left row (coalesced loads of a / b and their validity words)
template <int T>
__global__ __launch_bounds__(BLOCK) void k_rj_bounds(const RjBounds g) {
  __shared__ uint64_t s_keys[RJ_SAMPLES];
  for (uint32_t j = threadIdx.x; j < g.ns; j += BLOCK) s_keys[j] = g.keys[(uint64_t)j * g.stride];
  __syncthreads();
  for (int64_t base = (int64_t)blockIdx.x * BLOCK; base < g.nl; base += (int64_t)gridDim.x * BLOCK) {  // (wave-uniform: rj_diff_add votes)
    const int64_t l = base + threadIdx.x;
    const bool in = l < g.nl;
    bool bounded = in;
    uint32_t lo = 0, hi = g.m;
    if (in && g.a) {
      if (g.a_valid && !bit_at(g.a_valid, l)) bounded = false;
      else lo = rj_position<T>(g, s_keys, g.a, l, !g.lower_inclusive);
    }
    if (bounded && g.b) {
      if (g.b_valid && !bit_at(g.b_valid, l)) bounded = false;
      else hi = rj_position<T>(g, s_keys, g.b, l, g.upper_inclusive != 0);
    }
    const uint32_t cnt = bounded && hi > lo ? hi - lo : 0u;
    if (in) {
      g.lo[l] = lo;
      g.count[l] = cnt;
      g.visited[l] = cnt ? 1 : 0;
    }
    if (g.diff) {
      rj_diff_add(g.diff, cnt != 0, lo, 1);
      rj_diff_add(g.diff, cnt != 0, hi, -1);
    }
  }
}

// sorted position p is covered by cover[p + 1] runs (the exclusive prefix of the difference array, low 32 bits: its -1 entries were
// summed as 2^32 - 1); the hit byte goes to the row at that position
__global__ __launch_bounds__(BLOCK) void k_rj_cover(const uint64_t* __restrict__ cover, const uint32_t* __restrict__ perm, uint32_t m, uint8_t* __restrict__ hit) {
  for (int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x; p < m; p += (int64_t)gridDim.x * BLOCK)
    if ((int32_t)(uint32_t)cover[p + 1] > 0) hit[perm[p]] = 1;
}

struct RjExpand {
  const uint64_t* offsets;     // [nl + 1] exclusive prefix of the runs' lengths = the first output slot of every left row
  const uint32_t* lo;          // [nl]
  const uint32_t* perm;        // [m] right row at a sorted position
  uint32_t nl;
  int64_t total;
  int64_t* out_l;
  int64_t* out_r;
};

// A workgroup owns RJ_TILE consecutive output slots whatever rows they belong to: one left row that matches everything is written by
// as many workgroups as a million rows with one match each, and rows without a match cost nothing.  The tile's first and last row are
// found in the offsets; when the rows between them are at most RJ_TILE their offsets are staged (relative to the tile) and every slot
// finds its row in LDS, else (many rows without a match in between) in the offsets themselves.  Stores are coalesced: lane t writes
// slots t, t + BLOCK, ...
__global__ __launch_bounds__(BLOCK) void k_rj_expand(const RjExpand g) {
  __shared__ uint32_t s_off[RJ_TILE];
  __shared__ uint32_t s_row[2];
  const int64_t n_tiles = (g.total + RJ_TILE - 1) / RJ_TILE;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RJ_TILE, t1 = t0 + RJ_TILE < g.total ? t0 + RJ_TILE : g.total;
    // the row of slot j is the first l with offsets[l + 1] > j
    if (threadIdx.x < 2) s_row[threadIdx.x] = rj_search<true>(g.offsets + 1, 0u, g.nl, (uint64_t)(threadIdx.x ? t1 - 1 : t0));
    __syncthreads();
    const uint32_t r0 = s_row[0], nrows = s_row[1] - r0 + 1;
    const bool staged = nrows <= (uint32_t)RJ_TILE;
    if (staged)
      for (uint32_t i = threadIdx.x; i < nrows; i += BLOCK) {
        const uint64_t o = g.offsets[(uint64_t)r0 + 1 + i] - (uint64_t)t0;
        s_off[i] = o < (uint64_t)RJ_TILE ? (uint32_t)o : (uint32_t)RJ_TILE;
      }
    __syncthreads();
    for (int64_t j = t0 + threadIdx.x; j < t1; j += BLOCK) {
      const uint32_t l = r0 + (staged ? rj_search<true>(s_off, 0u, nrows, (uint32_t)(j - t0)) : rj_search<true>(g.offsets + 1 + r0, 0u, nrows, (uint64_t)j));
      g.out_l[j] = l;
      g.out_r[j] = g.perm[g.lo[l] + (uint32_t)((uint64_t)j - g.offsets[l])];
    }
    __syncthreads();  // s_row / s_off are rewritten for the next tile
  }
}

namespace {

int rj_type(int t) {
  switch (t) {
    case DFGPU_INT32: case DFGPU_DATE32: return RJ_I32;
    case DFGPU_UINT32: return RJ_U32;
    case DFGPU_INT64: return RJ_I64;
    case DFGPU_UINT64: return RJ_U64;
    case DFGPU_FLOAT64: return RJ_F64;
  }
  return -1;
}
template <class F>
void with_rj_type(int t, F&& f) {
  switch (t) {
    case RJ_I32: f(std::integral_constant<int, RJ_I32>{}); break;
    case RJ_U32: f(std::integral_constant<int, RJ_U32>{}); break;
    case RJ_I64: f(std::integral_constant<int, RJ_I64>{}); break;
    case RJ_U64: f(std::integral_constant<int, RJ_U64>{}); break;
    default: f(std::integral_constant<int, RJ_F64>{}); break;
  }
}
void rj_check_key(const Column& c) {
  DFGPU_CHECK(!c.dict, "a range join key that is dictionary-encoded is not supported on the GPU path");
  DFGPU_CHECK(rj_type(c.field.type) >= 0, "a range join key of a type other than Int32, Int64, Date32, UInt32, UInt64 or Float64 is not supported on the GPU path");
}

}  // namespace

Table range_join(const Table& left, const Table& right, int jt, int x_col, int a_col, bool a_inclusive, int b_col, bool b_inclusive, const std::vector<int>& lout,
                 const std::vector<int>& rout) {
  DFGPU_CHECK(left.device == right.device, "the right table lives on another device than the left table (move it with dfgpu_table_copy_to_device)");
  for (int c : lout) DFGPU_CHECK(c >= 0 && c < (int)left.cols.size(), "left output column out of range");
  for (int c : rout) DFGPU_CHECK(c >= 0 && c < (int)right.cols.size(), "right output column out of range");
  DFGPU_CHECK(a_col >= 0 || b_col >= 0, "a range join needs a lower or an upper bound");
  DFGPU_CHECK(x_col >= 0 && x_col < (int)right.cols.size(), "range join key column out of range");
  DFGPU_CHECK(a_col < (int)left.cols.size() && b_col < (int)left.cols.size(), "range join bound column out of range");
  const Column& x = right.cols[x_col];
  const Column* a = a_col >= 0 ? &left.cols[a_col] : nullptr;
  const Column* b = b_col >= 0 ? &left.cols[b_col] : nullptr;
  rj_check_key(x);
  if (a) rj_check_key(*a);
  if (b) rj_check_key(*b);
  DFGPU_CHECK((!a || a->field.type == x.field.type) && (!b || b->field.type == x.field.type), "a range join over keys of different types is not supported on the GPU path");
  const int64_t nl = left.nrows, nr = right.nrows;
  DFGPU_CHECK(nl < ((int64_t)1 << 31) && nr < ((int64_t)1 << 31), "a range join side of 2^31 rows or more is not supported on the GPU path");

  Runtime& r = rt();
  const int T = rj_type(x.field.type), w = type_width(x.field.type);
  const bool right_flags = jt == DFGPU_JOIN_RIGHT || jt == DFGPU_JOIN_FULL || right_one_sided(jt);
  NljMatches M;
  M.hit = make_zero_buf((size_t)nr + 64);
  M.visited = make_zero_buf((size_t)nl + 64);
  BufPtr prefix, key, perm, lo, counts, offsets;
  int64_t m = 0, n_pass = 0;
  if (nl && nr) {
    // ---- keys: the non-NULL x as (ordered key - its minimum, row), sorted by the bits the span needs
    m = nr;
    if (x.validity) {
      const int64_t nw = (nr + 63) / 64;
      prefix = make_buf((size_t)(nw + 1) * 8);
      scan_mask_popcounts(x.valid_words(), nullptr, nr, prefix->as<uint64_t>());
      m = (int64_t)read_u64(prefix->as<uint64_t>() + nw);
    }
  }
  if (m) {
    uint64_t base = 0, span = ~0ull;
    if (T != RJ_U64 && T != RJ_F64) {  // (column_stats keeps signed 64-bit bounds: not UInt64's, and Float64 has no integer order)
      const ColStats st = column_stats(const_cast<Column&>(x), nr);  // fills the column's shared cache; the rows do not change
      const uint64_t flip = T == RJ_U32 ? 0ull : 1ull << 63;
      base = (uint64_t)st.min ^ flip;
      span = ((uint64_t)st.max ^ flip) - base;  // in u64: INT64_MAX - INT64_MIN is 2^64 - 1
    }
    const int nbits = span ? 64 - __builtin_clzll(span) : 0;
    key = make_buf((size_t)m * 8);
    if (x.validity) perm = make_buf((size_t)m * 4);
    {
      ProfileScope ps("rangejoin_keys", nr * w + m * (x.validity ? 12 : 8));
      with_rj_type(T, [&](auto t) {
        k_rj_keys<decltype(t)::value><<<grid_for(nr, BLOCK), BLOCK, 0, r.stream>>>(x.ptr(), x.valid_words(), prefix ? prefix->as<uint64_t>() : nullptr, nr, base,
                                                                                  key->as<uint64_t>(), perm ? perm->as<uint32_t>() : nullptr);
      });
      DFGPU_HIP(hipGetLastError());
    }
    radix_sort_pairs(key, perm, m, 0, nbits);  // stable: equal x keep ascending row order

    // ---- bounds: every left row's run of the sorted order
    lo = make_buf((size_t)nl * 4);
    counts = make_buf((size_t)nl * 4);
    BufPtr diff = right_flags ? make_zero_buf((size_t)(m + 1) * 4) : nullptr;
    RjBounds g{};
    g.a = a ? a->ptr() : nullptr;
    g.a_valid = a ? a->valid_words() : nullptr;
    g.b = b ? b->ptr() : nullptr;
    g.b_valid = b ? b->valid_words() : nullptr;
    g.lower_inclusive = a_inclusive;
    g.upper_inclusive = b_inclusive;
    g.nl = nl;
    g.keys = key->as<uint64_t>();
    g.m = (uint32_t)m;
    g.stride = (uint32_t)((m + RJ_SAMPLES - 1) / RJ_SAMPLES);
    g.ns = (uint32_t)((m + g.stride - 1) / g.stride);
    g.base = base;
    g.span = span;
    g.lo = lo->as<uint32_t>();
    g.count = counts->as<uint32_t>();
    g.visited = M.visited->as<uint8_t>();
    g.diff = diff ? diff->as<int32_t>() : nullptr;
    {
      ProfileScope ps("rangejoin_bounds", nl * ((a ? w : 0) + (b ? w : 0) + 9) + (diff ? m * 4 : 0));
      with_rj_type(T, [&](auto t) { k_rj_bounds<decltype(t)::value><<<grid_for(nl, BLOCK), BLOCK, 0, r.stream>>>(g); });
      DFGPU_HIP(hipGetLastError());
    }
    // ---- coverage: which right rows lie in some run
    if (right_flags) {
      BufPtr cover = make_buf((size_t)(m + 1) * 8);
      scan_u32(reinterpret_cast<const uint32_t*>(diff->as<int32_t>()), m, cover->as<uint64_t>());
      ProfileScope ps("rangejoin_cover", m * 12 + m);
      k_rj_cover<<<grid_for(m, BLOCK), BLOCK, 0, r.stream>>>(cover->as<uint64_t>(), perm->as<uint32_t>(), (uint32_t)m, M.hit->as<uint8_t>());
      DFGPU_HIP(hipGetLastError());
    }
    if (pairs_out(jt)) {
      offsets = make_buf((size_t)(nl + 1) * 8);
      scan_u32(counts->as<uint32_t>(), nl, offsets->as<uint64_t>());
      n_pass = (int64_t)read_u64(offsets->as<uint64_t>() + nl);
    }
  }
  return nlj_tail(left, right, jt, lout, rout, M, n_pass, [&](int64_t* pl, int64_t* pr) {
    if (!n_pass) return;
    const RjExpand e{offsets->as<uint64_t>(), lo->as<uint32_t>(), perm->as<uint32_t>(), (uint32_t)nl, n_pass, pl, pr};
    const int64_t n_tiles = (n_pass + RJ_TILE - 1) / RJ_TILE;
    ProfileScope ps("rangejoin_expand", n_pass * 20 + nl * 12);
    k_rj_expand<<<(unsigned)std::min<int64_t>(n_tiles, (int64_t)policy().num_cus * 32), BLOCK, 0, r.stream>>>(e);
    DFGPU_HIP(hipGetLastError());
  });
}

}  // namespace dfgpu

using namespace dfgpu;

int dfgpu_nested_loop_join(dfgpu_table_t left, dfgpu_table_t right, int join_type, const dfgpu_join_filter* filter, const int* left_out_cols, int n_left_out,
                           const int* right_out_cols, int n_right_out, dfgpu_table_t* out) {
  return guarded([&] {
    require_init();
    DFGPU_CHECK(left && right && out && n_left_out >= 0 && n_right_out >= 0 && (!filter || filter->n_columns >= 0), "null argument");
    DFGPU_CHECK(join_type >= DFGPU_JOIN_INNER && join_type <= DFGPU_JOIN_RIGHT_MARK, "bad join type");
    const Table* lt = unwrap(left);
    const Table* rtb = unwrap(right);
    std::vector<int> lo(left_out_cols, left_out_cols + n_left_out), ro(right_out_cols, right_out_cols + n_right_out);
    auto o = std::make_unique<Table>(nested_loop_join(*lt, *rtb, join_type, filter, lo, ro));
    *out = wrap(o.release());
  });
}

int dfgpu_range_join(dfgpu_table_t left, dfgpu_table_t right, int join_type, int right_key_col, int lower_col, int lower_inclusive, int upper_col, int upper_inclusive,
                     const int* left_out_cols, int n_left_out, const int* right_out_cols, int n_right_out, dfgpu_table_t* out) {
  return guarded([&] {
    require_init();
    DFGPU_CHECK(left && right && out && n_left_out >= 0 && n_right_out >= 0 && (left_out_cols || !n_left_out) && (right_out_cols || !n_right_out), "null argument");
    DFGPU_CHECK(join_type >= DFGPU_JOIN_INNER && join_type <= DFGPU_JOIN_RIGHT_MARK, "bad join type");
    const Table* lt = unwrap(left);
    const Table* rtb = unwrap(right);
    std::vector<int> lo, ro;
    if (n_left_out) lo.assign(left_out_cols, left_out_cols + n_left_out);
    if (n_right_out) ro.assign(right_out_cols, right_out_cols + n_right_out);
    auto o = std::make_unique<Table>(range_join(*lt, *rtb, join_type, right_key_col, lower_col < 0 ? -1 : lower_col, lower_inclusive != 0, upper_col < 0 ? -1 : upper_col,
                                                upper_inclusive != 0, lo, ro));
    *out = wrap(o.release());
  });
}
