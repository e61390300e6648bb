// window.hip — WindowAggExec / BoundedWindowAggExec over input that arrives ordered by (partition keys, order keys): ranking
// functions and running aggregates.  No table, no hashing: boundaries are marked, everything else is a segmented scan.
//   heads    : one pass over the key columns writes TWO bitmaps, one bit per row in 64-row words (the k_run_heads idiom of the
//              ordered-input aggregate, NULL-aware and over several columns): partition heads, and peer heads (a partition head, or
//              an order column that differs from the row before)
//   starts   : "position of the last head at or before this row" = an unsegmented max scan of (head ? row : -inf);
//   ends     : "last row before the next head" = the same as a min scan over the rows in reverse
//   scan     : device-wide SEGMENTED inclusive scan of the argument under the partition heads — (value, count of non-NULL values)
//              pairs under add (u64 / i128 / f64) or min / max (i64 / i128).  Reduce / carry / down-sweep like scan.hip's three-launch
//              form: per-tile (aggregate, any-head) pairs, ONE workgroup scans the tile carries, the down-sweep scans each tile again
//              from its carry.  No workgroup waits on another (why this scan does not chain).
//   finish   : the output row takes the scanned pair at its own row (ROWS frame), at its last peer (RANGE frame) or at the
//              partition's last row, and turns it into the result type and a validity bit.  When every peer-head bit is set (a
//              popcount tells) RANGE is ROWS and the pick is skipped.
// A Float64 sum is a tree of additions over exactly its frame's values (identity 0.0 joins exactly): never a difference of prefixes.
//
// PERCENT_RANK / CUME_DIST / NTILE and FIRST_VALUE / LAST_VALUE / NTH_VALUE (ABI 18) take a row's positions from the bitmaps themselves:
//   words    : per head bitmap two arrays of one int64 per 64-row WORD — last_upto[w] = the row of the last head in words 0..w (the max
//              scan above over n_words elements), first_from[w] = the row of the first head in words w.., or n (the min scan in reverse)
//   start(i) : w = i >> 6, b = i & 63;  m = heads[w] & (~0ull >> (63 - b));
//              m ? (w << 6) + 63 - clz(m) : last_upto[w - 1]          // row 0 is always a head: w == 0 never falls through
//   end(i)   : m = b == 63 ? 0 : heads[w] & (~0ull << (b + 1));        // never shift by 64
//              next = m ? (w << 6) + ctz(m) : (w + 1 < n_words ? first_from[w + 1] : n);   return next - 1
//   dist     : one wave per word; the bitmap word and the two summary entries are one address per wave, 8 bytes are written per row
//   value    : the same loop; the row picks one row of its frame, gathers the argument there and ballots the validity word
// No n * 8 position array is built for them.  With s / e the first / last row of the row's partition, rows = e - s + 1, ps / pe the
// first / last row of its peer group and i the row itself (DataFusion 55 functions-window: rank.rs, cume_dist.rs, ntile.rs, nth_value.rs):
//   percent_rank  (double)(ps - s) / (double)max(rows - 1, 1)                                     Float64, never NULL
//   cume_dist     (double)(pe - s + 1) / (double)rows                                             Float64, never NULL
//   ntile(n)      n >= 1; k = min(n, rows); (i - s) * k / rows + 1 (unsigned 64-bit, truncating)  UInt64, never NULL
// The value functions are RESPECT NULLS over the frame [s, f]: f = i (rows_to_current), f = pe (range_to_current), f = e (partition):
//   first_value          the argument at s
//   last_value           the argument at f
//   nth_value(n), n > 0  the argument at s + n - 1 if that is <= f, otherwise NULL
//   nth_value(n), n < 0  the argument at f + n + 1 if that is >= s, otherwise NULL
// A NULL argument at the picked row gives NULL; the value slot under a NULL result is 0.
#include <climits>

#include "device.hpp"
#include "internal.hpp"

namespace dfgpu {

constexpr int WIN_ITEMS = 8;
constexpr int WIN_TILE = BLOCK * WIN_ITEMS;   // rows per workgroup
static_assert(WIN_TILE == DFGPU_WINDOW_TILE, "include/dfgpu.h names the tile size");

// ------------------------------------------------------------------------------------------------ heads
// row i against row i - 1 (i >= 1): validity differs, or both are valid and the value bits differ.  Two NULLs are equal whatever
// their value slots hold.
__device__ __forceinline__ bool win_keys_differ(const KeySet& ks, int64_t i) {
  for (int c = 0; c < ks.n; c++) {
    const KeyCol& k = ks.c[c];
    const bool va = !k.valid || bit_at(k.valid, i), vb = !k.valid || bit_at(k.valid, i - 1);
    if (va != vb) return true;
    if (!va) continue;
    uint64_t alo, ahi, blo, bhi;
    load_words(k, i, alo, ahi);
    load_words(k, i - 1, blo, bhi);
    if (alo != blo || ahi != bhi) return true;
  }
  return false;
}
__global__ __launch_bounds__(BLOCK) void k_window_heads(KeySet part, KeySet order, int64_t n, uint64_t* __restrict__ part_heads, uint64_t* __restrict__ peer_heads) {
  const int64_t n_words = (n + 63) >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * BLOCK) >> 6;
  for (int64_t w = wave; w < n_words; w += n_waves) {
    const int64_t i = (w << 6) + lane_id();
    bool ph = false, oh = false;
    if (i < n) {
      ph = i == 0 || win_keys_differ(part, i);
      oh = ph || win_keys_differ(order, i);
    }
    const uint64_t a = ballot64(ph), b = ballot64(oh);
    if (lane_id() == 0) {
      part_heads[w] = a;
      peer_heads[w] = b;
    }
  }
}
// set bits of a bitmap whose bits beyond the last row are clear
__global__ __launch_bounds__(BLOCK) void k_window_popcount(const uint64_t* __restrict__ bits, int64_t n_words, unsigned long long* __restrict__ total) {
  unsigned long long s = 0;
  for (int64_t w = (int64_t)blockIdx.x * BLOCK + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * BLOCK) s += (unsigned)__popcll(bits[w]);
  s = wave_sum(s);
  if (lane_id() == 0 && s) atomicAdd(total, s);
}

// ------------------------------------------------------------------------------------------------ the scanned pair
template <typename V>
struct WVal {
  V v;          // the operator's running value over the non-NULL rows
  uint64_t c;   // how many of them
};
// (f64_ordered / f64_from_ordered of the aggregate, restated: IEEE totalOrder as a signed integer, an involution on the bits)
__device__ __forceinline__ int64_t win_f64_ordered(int64_t b) { return b ^ (int64_t)((uint64_t)(b >> 63) >> 1); }

struct OpAddU64 {
  typedef uint64_t V;
  static __device__ __forceinline__ V ident() { return 0; }
  static __device__ __forceinline__ V make(uint64_t lo, uint64_t) { return lo; }
  static __device__ __forceinline__ V comb(V a, V b) { return a + b; }
};
struct OpAddI128 {
  typedef u128 V;
  static __device__ __forceinline__ V ident() { return 0; }
  static __device__ __forceinline__ V make(uint64_t lo, uint64_t hi) { return ((u128)hi << 64) | lo; }
  static __device__ __forceinline__ V comb(V a, V b) { return a + b; }
};
struct OpAddF64 {
  typedef double V;
  static __device__ __forceinline__ V ident() { return 0.0; }
  static __device__ __forceinline__ V make(uint64_t lo, uint64_t) { return __longlong_as_double((long long)lo); }
  static __device__ __forceinline__ V comb(V a, V b) { return a + b; }
};
struct OpMinI64 {
  typedef int64_t V;
  static __device__ __forceinline__ V ident() { return INT64_MAX; }
  static __device__ __forceinline__ V make(uint64_t lo, uint64_t) { return (int64_t)lo; }
  static __device__ __forceinline__ V comb(V a, V b) { return b < a ? b : a; }
};
struct OpMaxI64 {
  typedef int64_t V;
  static __device__ __forceinline__ V ident() { return INT64_MIN; }
  static __device__ __forceinline__ V make(uint64_t lo, uint64_t) { return (int64_t)lo; }
  static __device__ __forceinline__ V comb(V a, V b) { return b > a ? b : a; }
};
struct OpMinI128 {
  typedef i128 V;
  static __device__ __forceinline__ V ident() { return (i128)(~(u128)0 >> 1); }
  static __device__ __forceinline__ V make(uint64_t lo, uint64_t hi) { return (i128)(((u128)hi << 64) | lo); }
  static __device__ __forceinline__ V comb(V a, V b) { return b < a ? b : a; }
};
struct OpMaxI128 {
  typedef i128 V;
  static __device__ __forceinline__ V ident() { return (i128)((u128)1 << 127); }
  static __device__ __forceinline__ V make(uint64_t lo, uint64_t hi) { return (i128)(((u128)hi << 64) | lo); }
  static __device__ __forceinline__ V comb(V a, V b) { return b > a ? b : a; }
};
template <class Op>
__device__ __forceinline__ WVal<typename Op::V> wv_ident() {
  WVal<typename Op::V> r;
  r.v = Op::ident();
  r.c = 0;
  return r;
}
template <class Op>
__device__ __forceinline__ WVal<typename Op::V> wv_comb(const WVal<typename Op::V>& a, const WVal<typename Op::V>& b) {  // a = the earlier rows
  WVal<typename Op::V> r;
  r.v = Op::comb(a.v, b.v);
  r.c = a.c + b.c;
  return r;
}
template <typename T>
__device__ __forceinline__ T shfl_up_any(const T& x, int d) {
  static_assert(sizeof(T) % 4 == 0, "shuffled by 32-bit words");
  constexpr int N = sizeof(T) / 4;
  union U {
    T t;
    int w[N];
    __device__ U() {}
  } a, b;
  a.t = x;
#pragma unroll
  for (int k = 0; k < N; k++) b.w[k] = __shfl_up(a.w[k], d, 64);
  return b.t;
}

// what a scan reads per row
enum WinSrc : int {
  WS_I32 = 0, WS_I64 = 1, WS_U8 = 2, WS_U32 = 3, WS_F64 = 4, WS_F64_ORDERED = 5, WS_I128 = 6, WS_I32_TO_F64 = 7, WS_I64_TO_F64 = 8,
  WS_NONE = 9,       // no value: COUNT (the validity alone) and ROW_NUMBER-like counts
  WS_BIT = 10,       // `bits`[row] as 0 / 1 (DENSE_RANK: the peer heads)
  WS_START_POS = 11, // `bits`[row] ? row : -inf         (max scan: the last head at or before the row)
  WS_END_POS = 12,   // row is the last or `bits`[row + 1] ? row : +inf   (min scan in reverse: the last row before the next head)
  // over the WORDS of `bits` (n = the number of words):
  WS_WORD_START = 13, // `bits`[w] ? the row of its highest set bit : -inf   (max scan: the last head in words 0..w)
  WS_WORD_END = 14    // `bits`[w] ? the row of its lowest set bit : +inf, the last word's no more than `limit`   (min scan in reverse: the
                      // first head in words w.., or `limit` = the number of rows)
};
struct WinIn {
  const void* data;
  const uint64_t* valid;   // the argument's validity (null = no NULLs)
  const uint64_t* heads;   // segment heads (null = one segment)
  const uint64_t* bits;    // WS_BIT / WS_START_POS / WS_END_POS
  int64_t n;
  int src;
  int reverse;             // scan position i is row n - 1 - i (heads must be null)
  int64_t limit;           // WS_WORD_END
};
__device__ __forceinline__ int64_t win_row(const WinIn& in, int64_t i) { return in.reverse ? in.n - 1 - i : i; }
__device__ __forceinline__ bool win_head(const WinIn& in, int64_t i) { return in.heads && bit_at(in.heads, i); }
// the pair of scan position i (< n): the identity with count 0 under a NULL — its value slot is never read
template <class Op>
__device__ __forceinline__ WVal<typename Op::V> win_load(const WinIn& in, int64_t i) {
  const int64_t e = win_row(in, i);
  WVal<typename Op::V> r = wv_ident<Op>();
  if (in.valid && !bit_at(in.valid, e)) return r;
  r.c = 1;
  uint64_t lo = 0, hi = 0;
  switch (in.src) {
    case WS_I32: lo = (uint64_t)(int64_t)((const int32_t*)in.data)[e]; hi = (uint64_t)((int64_t)lo >> 63); break;
    case WS_I64: lo = ((const uint64_t*)in.data)[e]; hi = (uint64_t)((int64_t)lo >> 63); break;
    case WS_U8: lo = ((const uint8_t*)in.data)[e]; break;
    case WS_U32: lo = ((const uint32_t*)in.data)[e]; break;
    case WS_F64: lo = ((const uint64_t*)in.data)[e]; break;
    case WS_F64_ORDERED: lo = (uint64_t)win_f64_ordered(((const int64_t*)in.data)[e]); break;
    case WS_I128: lo = ((const uint64_t*)in.data)[2 * e]; hi = ((const uint64_t*)in.data)[2 * e + 1]; break;
    case WS_I32_TO_F64: lo = (uint64_t)__double_as_longlong((double)((const int32_t*)in.data)[e]); break;
    case WS_I64_TO_F64: lo = (uint64_t)__double_as_longlong((double)((const int64_t*)in.data)[e]); break;
    case WS_NONE: return r;
    case WS_BIT: lo = bit_at(in.bits, e) ? 1 : 0; break;
    case WS_START_POS: lo = (uint64_t)(bit_at(in.bits, e) ? e : INT64_MIN); break;
    case WS_END_POS: lo = (uint64_t)((e == in.n - 1 || bit_at(in.bits, e + 1)) ? e : INT64_MAX); break;
    case WS_WORD_START: {
      const uint64_t b = in.bits[e];
      lo = (uint64_t)(b ? (e << 6) + 63 - __clzll((long long)b) : INT64_MIN);
      break;
    }
    case WS_WORD_END: {
      const uint64_t b = in.bits[e];
      int64_t x = b ? (e << 6) + __ffsll((unsigned long long)b) - 1 : INT64_MAX;
      if (e == in.n - 1 && x > in.limit) x = in.limit;
      lo = (uint64_t)x;
      break;
    }
  }
  r.v = Op::make(lo, hi);
  return r;
}

// Segmented scan over the BLOCK threads' (aggregate, any-head) pairs.  `ex` / `ex_f` = the pair of everything before this thread in the
// workgroup, `total` / `total_f` = the workgroup's own.  Wave level: Hillis-Steele over shuffles; the four wave totals meet in LDS.
template <class Op>
__device__ __forceinline__ void block_seg_scan(WVal<typename Op::V> a, bool f, WVal<typename Op::V>& ex, bool& ex_f, WVal<typename Op::V>& total, bool& total_f) {
  typedef WVal<typename Op::V> P;
  __shared__ P s_a[BLOCK / WAVE];
  __shared__ int s_f[BLOCK / WAVE];
  const int lane = (int)lane_id(), w = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const P o = shfl_up_any(a, d);
    const int fo = __shfl_up((int)f, d, 64);
    if (lane >= d) {
      if (!f) a = wv_comb<Op>(o, a);
      f = f || fo != 0;
    }
  }
  if (lane == 63) {
    s_a[w] = a;
    s_f[w] = f;
  }
  P prev = shfl_up_any(a, 1);
  bool prev_f = __shfl_up((int)f, 1, 64) != 0;
  if (lane == 0) {
    prev = wv_ident<Op>();
    prev_f = false;
  }
  __syncthreads();
  P p = wv_ident<Op>(), before = p;
  bool pf = false, before_f = false;
#pragma unroll
  for (int k = 0; k < BLOCK / WAVE; k++) {
    if (k == w) {
      before = p;
      before_f = pf;
    }
    if (s_f[k]) {
      p = s_a[k];
      pf = true;
    } else {
      p = wv_comb<Op>(p, s_a[k]);
    }
  }
  total = p;
  total_f = pf;
  ex = prev_f ? prev : wv_comb<Op>(before, prev);
  ex_f = prev_f || before_f;
  __syncthreads();   // s_a / s_f are reused by the next call
}

// per tile: its (aggregate, any-head) pair
template <class Op>
__global__ __launch_bounds__(BLOCK) void k_window_reduce(WinIn in, WVal<typename Op::V>* __restrict__ tile_a, uint8_t* __restrict__ tile_f) {
  typedef WVal<typename Op::V> P;
  const int64_t base = (int64_t)blockIdx.x * WIN_TILE + (int64_t)threadIdx.x * WIN_ITEMS;
  P a = wv_ident<Op>();
  bool f = false;
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; j++) {
    const int64_t i = base + j;
    if (i < in.n) {
      const P x = win_load<Op>(in, i);
      if (win_head(in, i)) {
        a = x;
        f = true;
      } else {
        a = wv_comb<Op>(a, x);
      }
    }
  }
  P ex, total;
  bool ex_f, total_f;
  block_seg_scan<Op>(a, f, ex, ex_f, total, total_f);
  if (threadIdx.x == 0) {
    tile_a[blockIdx.x] = total;
    tile_f[blockIdx.x] = total_f ? 1 : 0;
  }
}
// ONE workgroup: the tile pairs become each tile's carry (the pair of the rows between the last head before the tile and the tile), in
// place, BLOCK tiles per round; `run` carries the scan from one round to the next
template <class Op>
__global__ __launch_bounds__(BLOCK) void k_window_carry(WVal<typename Op::V>* __restrict__ tile_a, const uint8_t* __restrict__ tile_f, int64_t n_tiles) {
  typedef WVal<typename Op::V> P;
  P run = wv_ident<Op>();
  for (int64_t base = 0; base < n_tiles; base += BLOCK) {
    const int64_t t = base + threadIdx.x;
    const bool live = t < n_tiles;
    const P a = live ? tile_a[t] : wv_ident<Op>();
    const bool f = live && tile_f[t] != 0;
    P ex, total;
    bool ex_f, total_f;
    block_seg_scan<Op>(a, f, ex, ex_f, total, total_f);
    if (live) tile_a[t] = ex_f ? ex : wv_comb<Op>(run, ex);
    run = total_f ? total : wv_comb<Op>(run, total);
  }
}
// per tile: the scan itself, from the tile's carry; out_v / out_c are indexed by ROW (a reverse scan writes back to front)
template <class Op>
__global__ __launch_bounds__(BLOCK) void k_window_down(WinIn in, const WVal<typename Op::V>* __restrict__ tile_carry, typename Op::V* __restrict__ out_v,
                                                       uint64_t* __restrict__ out_c) {
  typedef WVal<typename Op::V> P;
  const int64_t base = (int64_t)blockIdx.x * WIN_TILE + (int64_t)threadIdx.x * WIN_ITEMS;
  P x[WIN_ITEMS];
  bool h[WIN_ITEMS];
  P a = wv_ident<Op>();
  bool f = false;
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; j++) {
    const int64_t i = base + j;
    x[j] = wv_ident<Op>();
    h[j] = false;
    if (i < in.n) {
      x[j] = win_load<Op>(in, i);
      h[j] = win_head(in, i);
      if (h[j]) {
        a = x[j];
        f = true;
      } else {
        a = wv_comb<Op>(a, x[j]);
      }
    }
  }
  P ex, total;
  bool ex_f, total_f;
  block_seg_scan<Op>(a, f, ex, ex_f, total, total_f);
  P r = ex_f ? ex : wv_comb<Op>(tile_carry[blockIdx.x], ex);
#pragma unroll
  for (int j = 0; j < WIN_ITEMS; j++) {
    const int64_t i = base + j;
    if (i < in.n) {
      r = h[j] ? x[j] : wv_comb<Op>(r, x[j]);
      const int64_t e = win_row(in, i);
      out_v[e] = r.v;
      if (out_c) out_c[e] = r.c;
    }
  }
}

// ------------------------------------------------------------------------------------------------ finish
enum WinFin : int {
  WF_COPY8 = 0,    // 64-bit value as it is (sums, Int64 / UInt64 MIN / MAX)
  WF_LOW4 = 1,     // its low 4 bytes (Int32 / Date32 / UInt32 MIN / MAX)
  WF_LOW1 = 2,     // its low byte (UInt8)
  WF_F64_ORDERED = 3,
  WF_COPY16 = 4,
  WF_COUNT = 5,    // the count itself, never NULL
  WF_AVG_F64 = 6,  // sum / count
  WF_AVG_DEC = 7   // (sum * mul) / count, truncating (DecimalAverager::avg); an overflowing product raises *overflow
};
// one wave per 64 rows: the row's pair is the scanned pair at pos[row] (PICK) or at the row itself; a frame without a non-NULL value
// gives NULL (a zeroed value slot and a clear validity bit)
template <bool PICK>
__global__ __launch_bounds__(BLOCK) void k_window_finish(const void* __restrict__ v, const uint64_t* __restrict__ c, const int64_t* __restrict__ pos, int fin, i128 mul,
                                                         int64_t n, void* __restrict__ out, uint64_t* __restrict__ out_valid, int* __restrict__ overflow) {
  const int64_t n_words = (n + 63) >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * BLOCK) >> 6;
  for (int64_t w = wave; w < n_words; w += n_waves) {
    const int64_t i = (w << 6) + lane_id();
    bool ok = false;
    if (i < n) {
      const int64_t p = PICK ? pos[i] : i;
      const uint64_t cnt = c[p];
      ok = cnt != 0 || fin == WF_COUNT;
      switch (fin) {
        case WF_COPY8: ((uint64_t*)out)[i] = ok ? ((const uint64_t*)v)[p] : 0; break;
        case WF_LOW4: ((uint32_t*)out)[i] = ok ? (uint32_t)((const uint64_t*)v)[p] : 0; break;
        case WF_LOW1: ((uint8_t*)out)[i] = ok ? (uint8_t)((const uint64_t*)v)[p] : 0; break;
        case WF_F64_ORDERED: ((int64_t*)out)[i] = ok ? win_f64_ordered(((const int64_t*)v)[p]) : 0; break;
        case WF_COPY16: ((u128*)out)[i] = ok ? ((const u128*)v)[p] : (u128)0; break;
        case WF_COUNT: ((uint64_t*)out)[i] = cnt; break;
        case WF_AVG_F64: ((double*)out)[i] = ok ? ((const double*)v)[p] / (double)cnt : 0.0; break;
        case WF_AVG_DEC: {
          i128 r = 0;
          if (ok) {
            if (__builtin_mul_overflow(((const i128*)v)[p], mul, &r)) *overflow = 1;
            r = r / (i128)cnt;
          }
          ((i128*)out)[i] = r;
          break;
        }
      }
    }
    const uint64_t b = ballot64(ok);
    if (lane_id() == 0 && out_valid) out_valid[w] = b;
  }
}
// ROW_NUMBER (mode 0) = row - partition start + 1, RANK (mode 1) = peer start - partition start + 1
__global__ __launch_bounds__(BLOCK) void k_window_rank(int mode, const int64_t* __restrict__ part_start, const int64_t* __restrict__ peer_start, int64_t n,
                                                       uint64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK)
    out[i] = (uint64_t)((mode == 0 ? i : peer_start[i]) - part_start[i] + 1);
}

// ------------------------------------------------------------------------------------------------ positions from bitmap words
// one head bitmap and its per-word summaries (null where the caller's mode does not read them)
struct WinWords {
  const uint64_t* heads;
  const int64_t* last_upto;    // [w] = the row of the last head in words 0..w
  const int64_t* first_from;   // [w] = the row of the first head in words w.., or n
};
// what one wave reads of a WinWords for its word w: one address per wave each
struct WinWordCtx {
  uint64_t bits;    // heads[w]
  int64_t before;   // last_upto[w - 1] (word 0: 0 — row 0 is always a head, it is never taken)
  int64_t after;    // first_from[w + 1], or n behind the last word
};
__device__ __forceinline__ WinWordCtx win_word_ctx(const WinWords& x, int64_t w, int64_t n_words, int64_t n, bool starts, bool ends) {
  WinWordCtx c;
  c.bits = x.heads[w];
  c.before = starts && w > 0 ? x.last_upto[w - 1] : 0;
  c.after = ends && w + 1 < n_words ? x.first_from[w + 1] : n;
  return c;
}
// the last head at or before row (w << 6) + b
__device__ __forceinline__ int64_t win_start(const WinWordCtx& c, int64_t w, int b) {
  const uint64_t m = c.bits & (~0ull >> (63 - b));
  return m ? (w << 6) + 63 - __clzll((long long)m) : c.before;
}
// the last row before the next head behind row (w << 6) + b
__device__ __forceinline__ int64_t win_end(const WinWordCtx& c, int64_t w, int b) {
  const uint64_t m = b == 63 ? 0 : c.bits & (~0ull << (b + 1));   // never shift by 64
  const int64_t next = m ? (w << 6) + __ffsll((unsigned long long)m) - 1 : c.after;
  return next - 1;
}

enum WinDist : int { WD_PERCENT_RANK = 0, WD_CUME_DIST = 1, WD_NTILE = 2 };
// one wave per 64 rows.  NTILE never touches the peer bitmap; PERCENT_RANK reads the peer starts, CUME_DIST the peer ends.
__global__ __launch_bounds__(BLOCK) void k_window_dist(int mode, WinWords part, WinWords peer, uint64_t buckets, int64_t n, void* __restrict__ out) {
  const int64_t n_words = (n + 63) >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * BLOCK) >> 6;
  for (int64_t w = wave; w < n_words; w += n_waves) {
    const int b = (int)lane_id();
    const int64_t i = (w << 6) + b;
    const WinWordCtx pc = win_word_ctx(part, w, n_words, n, true, true);
    WinWordCtx oc{};
    if (mode != WD_NTILE) oc = win_word_ctx(peer, w, n_words, n, mode == WD_PERCENT_RANK, mode == WD_CUME_DIST);
    if (i < n) {
      const int64_t s = win_start(pc, w, b), e = win_end(pc, w, b);
      const uint64_t rows = (uint64_t)(e - s + 1);
      if (mode == WD_NTILE) {
        const uint64_t k = buckets < rows ? buckets : rows;
        stream_store((uint64_t*)out + i, (uint64_t)(i - s) * k / rows + 1);
      } else if (mode == WD_PERCENT_RANK) {
        const int64_t ps = win_start(oc, w, b);
        stream_store((double*)out + i, (double)(ps - s) / (double)(rows > 1 ? rows - 1 : 1));
      } else {
        const int64_t pe = win_end(oc, w, b);
        stream_store((double*)out + i, (double)(pe - s + 1) / (double)rows);
      }
    }
  }
}

enum WinPick : int { WP_FIRST = 0, WP_LAST = 1, WP_NTH = 2 };
template <typename T>
__device__ __forceinline__ void win_store(T* p, T v) { stream_store(p, v); }
template <>
__device__ __forceinline__ void win_store<u128>(u128* p, u128 v) {
  stream_store((uint4*)p, make_uint4((unsigned)v, (unsigned)(v >> 32), (unsigned)(v >> 64), (unsigned)(v >> 96)));
}
template <int WIDTH> struct WinBytes;
template <> struct WinBytes<1> { typedef uint8_t T; };
template <> struct WinBytes<4> { typedef uint32_t T; };
template <> struct WinBytes<8> { typedef uint64_t T; };
template <> struct WinBytes<16> { typedef u128 T; };
// one wave per 64 rows: the row picks row p of its frame [s, f] (or none), the result is the argument's bytes there — unchanged,
// whatever they mean — or NULL (a zeroed value slot and a clear validity bit) where there is no p or the argument at p is NULL.
// `frame_ends` = the bitmap whose run ends are f (the peer heads: RANGE, the partition heads: PARTITION), null for ROWS (f = the row).
template <int WIDTH>
__global__ __launch_bounds__(BLOCK) void k_window_value(int pick, int64_t nth, WinWords part, WinWords frame_ends, const void* __restrict__ arg,
                                                        const uint64_t* __restrict__ valid, int64_t n, void* __restrict__ out, uint64_t* __restrict__ out_valid) {
  typedef typename WinBytes<WIDTH>::T T;
  const int64_t n_words = (n + 63) >> 6;
  const int64_t wave = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * BLOCK) >> 6;
  const bool need_s = pick != WP_LAST, need_f = pick != WP_FIRST;
  for (int64_t w = wave; w < n_words; w += n_waves) {
    const int b = (int)lane_id();
    const int64_t i = (w << 6) + b;
    WinWordCtx pc{}, fc{};
    if (need_s) pc = win_word_ctx(part, w, n_words, n, true, false);
    if (need_f && frame_ends.heads) fc = win_word_ctx(frame_ends, w, n_words, n, false, true);
    bool ok = false;
    if (i < n) {
      const int64_t s = need_s ? win_start(pc, w, b) : 0;
      const int64_t f = !need_f ? 0 : frame_ends.heads ? win_end(fc, w, b) : i;
      int64_t p = -1;
      if (pick == WP_FIRST) p = s;
      else if (pick == WP_LAST) p = f;
      else if (nth > 0) p = nth - 1 <= f - s ? s + (nth - 1) : -1;   // (compared as distances: s + nth cannot overflow)
      else p = -(nth + 1) <= f - s ? f + (nth + 1) : -1;
      ok = p >= 0 && (!valid || bit_at(valid, p));
      T v = 0;
      if (ok) v = ((const T*)arg)[p];
      win_store((T*)out + i, v);
    }
    const uint64_t bal = ballot64(ok);
    if (lane_id() == 0) out_valid[w] = bal;
  }
}

// ------------------------------------------------------------------------------------------------ host
template <class Op>
static void run_window_scan(const WinIn& in, void* out_v, uint64_t* out_c, const char* name, int64_t bytes) {
  typedef WVal<typename Op::V> P;
  Runtime& r = rt();
  const int64_t n_tiles = (in.n + WIN_TILE - 1) / WIN_TILE;
  DFGPU_CHECK(n_tiles > 0 && n_tiles < (int64_t)INT_MAX, "window input too large");
  BufPtr ta = make_buf((size_t)n_tiles * sizeof(P)), tf = make_buf((size_t)n_tiles);
  ProfileScope ps(name, bytes);
  k_window_reduce<Op><<<(unsigned)n_tiles, BLOCK, 0, r.stream>>>(in, ta->as<P>(), tf->as<uint8_t>());
  k_window_carry<Op><<<1, BLOCK, 0, r.stream>>>(ta->as<P>(), tf->as<uint8_t>(), n_tiles);
  k_window_down<Op><<<(unsigned)n_tiles, BLOCK, 0, r.stream>>>(in, ta->as<P>(), (typename Op::V*)out_v, out_c);
  DFGPU_HIP(hipGetLastError());
}

enum WinOp : int { WO_ADD_U64, WO_ADD_I128, WO_ADD_F64, WO_MIN_I64, WO_MAX_I64, WO_MIN_I128, WO_MAX_I128, WO_COUNT };
static void run_window_op(int op, const WinIn& in, void* out_v, uint64_t* out_c, int64_t bytes) {
  switch (op) {
    case WO_ADD_U64: return run_window_scan<OpAddU64>(in, out_v, out_c, "window_scan_add_u64", bytes);
    case WO_ADD_I128: return run_window_scan<OpAddI128>(in, out_v, out_c, "window_scan_add_i128", bytes);
    case WO_ADD_F64: return run_window_scan<OpAddF64>(in, out_v, out_c, "window_scan_add_f64", bytes);
    case WO_MIN_I64: return run_window_scan<OpMinI64>(in, out_v, out_c, "window_scan_min_i64", bytes);
    case WO_MAX_I64: return run_window_scan<OpMaxI64>(in, out_v, out_c, "window_scan_max_i64", bytes);
    case WO_MIN_I128: return run_window_scan<OpMinI128>(in, out_v, out_c, "window_scan_min_i128", bytes);
    case WO_MAX_I128: return run_window_scan<OpMaxI128>(in, out_v, out_c, "window_scan_max_i128", bytes);
    case WO_COUNT: return run_window_scan<OpAddU64>(in, out_v, out_c, "window_scan_count", bytes);
  }
  throw Error("unknown window scan");
}

static dfgpu_field wfld(int type, int p = 0, int s = 0, int nullable = 1) {
  dfgpu_field f{};
  f.type = type;
  f.precision = p;
  f.scale = s;
  f.nullable = nullable;
  return f;
}
static std::string win_type_name(const Column& c) {
  if (c.dict) return "a dictionary-encoded column";
  return c.field.type == DFGPU_UTF8 ? std::string("Utf8") : type_name(c.field);
}
static const char* win_func_name(int func) {
  switch (func) {
    case DFGPU_WINDOW_ROW_NUMBER: return "ROW_NUMBER";
    case DFGPU_WINDOW_RANK: return "RANK";
    case DFGPU_WINDOW_DENSE_RANK: return "DENSE_RANK";
    case DFGPU_WINDOW_SUM: return "SUM";
    case DFGPU_WINDOW_COUNT: return "COUNT";
    case DFGPU_WINDOW_MIN: return "MIN";
    case DFGPU_WINDOW_MAX: return "MAX";
    case DFGPU_WINDOW_AVG: return "AVG";
    case DFGPU_WINDOW_PERCENT_RANK: return "PERCENT_RANK";
    case DFGPU_WINDOW_CUME_DIST: return "CUME_DIST";
    case DFGPU_WINDOW_NTILE: return "NTILE";
    case DFGPU_WINDOW_FIRST_VALUE: return "FIRST_VALUE";
    case DFGPU_WINDOW_LAST_VALUE: return "LAST_VALUE";
    case DFGPU_WINDOW_NTH_VALUE: return "NTH_VALUE";
  }
  throw Error("unknown dfgpu_window_func " + std::to_string(func));
}

// what an aggregate window function scans and emits, given its argument: the GPU AggregateExec's types (aggregate.hip sum_type /
// avg_type / plan_for), with MIN / MAX over Decimal128 compared in 128 bits
struct WinPlan {
  int op, src, fin;
  dfgpu_field out;
  int velem;    // bytes per scanned value
  i128 mul = 1;
};
static WinPlan plan_window(int func, const Column* arg) {
  if (func == DFGPU_WINDOW_COUNT) return {WO_COUNT, WS_NONE, WF_COUNT, wfld(DFGPU_INT64, 0, 0, 0), 8};
  DFGPU_CHECK(arg != nullptr, std::string(win_func_name(func)) + " needs an argument");
  const dfgpu_field& t = arg->field;
  const auto refuse = [&]() -> WinPlan { throw Error(std::string(win_func_name(func)) + " over " + win_type_name(*arg) + " is not supported on the GPU path"); };
  if (arg->dict) return refuse();
  switch (func) {
    case DFGPU_WINDOW_SUM:
      switch (t.type) {
        case DFGPU_DECIMAL128: return {WO_ADD_I128, WS_I128, WF_COPY16, wfld(DFGPU_DECIMAL128, std::min(38, t.precision + 10), t.scale), 16};
        case DFGPU_INT32: return {WO_ADD_U64, WS_I32, WF_COPY8, wfld(DFGPU_INT64), 8};
        case DFGPU_INT64: return {WO_ADD_U64, WS_I64, WF_COPY8, wfld(DFGPU_INT64), 8};
        case DFGPU_UINT8: return {WO_ADD_U64, WS_U8, WF_COPY8, wfld(DFGPU_INT64), 8};
        case DFGPU_UINT32: return {WO_ADD_U64, WS_U32, WF_COPY8, wfld(DFGPU_UINT64), 8};
        case DFGPU_UINT64: return {WO_ADD_U64, WS_I64, WF_COPY8, wfld(DFGPU_UINT64), 8};
        case DFGPU_FLOAT64: return {WO_ADD_F64, WS_F64, WF_COPY8, wfld(DFGPU_FLOAT64), 8};
      }
      return refuse();
    case DFGPU_WINDOW_AVG:
      switch (t.type) {
        case DFGPU_DECIMAL128: {
          // avg_sum_data_type widens to Decimal256 beyond 38 digits (aggregate.hip avg_sum_type): the same refusal
          DFGPU_CHECK(t.precision + 13 <= 38, "AVG over " + type_name(t) + " accumulates in Decimal256 in the reference: not supported on the GPU path");
          WinPlan p{WO_ADD_I128, WS_I128, WF_AVG_DEC, wfld(DFGPU_DECIMAL128, std::min(38, t.precision + 4), std::min(38, t.scale + 4)), 16};
          for (int k = t.scale; k < p.out.scale; k++) p.mul *= 10;
          return p;
        }
        case DFGPU_INT32: return {WO_ADD_F64, WS_I32_TO_F64, WF_AVG_F64, wfld(DFGPU_FLOAT64), 8};
        case DFGPU_INT64: return {WO_ADD_F64, WS_I64_TO_F64, WF_AVG_F64, wfld(DFGPU_FLOAT64), 8};
        case DFGPU_FLOAT64: return {WO_ADD_F64, WS_F64, WF_AVG_F64, wfld(DFGPU_FLOAT64), 8};
      }
      return refuse();
    case DFGPU_WINDOW_MIN:
    case DFGPU_WINDOW_MAX: {
      const bool mn = func == DFGPU_WINDOW_MIN;
      const int o64 = mn ? WO_MIN_I64 : WO_MAX_I64;
      switch (t.type) {
        case DFGPU_INT32: case DFGPU_DATE32: return {o64, WS_I32, WF_LOW4, t, 8};
        case DFGPU_INT64: return {o64, WS_I64, WF_COPY8, t, 8};
        case DFGPU_UINT8: return {o64, WS_U8, WF_LOW1, t, 8};
        case DFGPU_UINT32: return {o64, WS_U32, WF_LOW4, t, 8};
        case DFGPU_FLOAT64: return {o64, WS_F64_ORDERED, WF_F64_ORDERED, t, 8};
        case DFGPU_DECIMAL128: return {mn ? WO_MIN_I128 : WO_MAX_I128, WS_I128, WF_COPY16, t, 16};
      }
      return refuse();   // (UInt64: the aggregate compares signed 64-bit words and refuses it too)
    }
  }
  throw Error("unknown dfgpu_window_func " + std::to_string(func));
}

static KeySet window_keys(const Table& in, const int* cols, int n) {
  DFGPU_CHECK(n >= 0 && n <= MAX_KEYS && (n == 0 || cols != nullptr), "a window takes at most 8 partition and 8 order columns");
  KeySet ks{};
  ks.n = n;
  for (int k = 0; k < n; k++) {
    DFGPU_CHECK(cols[k] >= 0 && cols[k] < (int)in.cols.size(), "window key column out of range");
    const Column& c = in.cols[(size_t)cols[k]];
    // Keys are compared by value bits plus validity.  Float64 keys are refused because how the reference treats +0.0 / -0.0 and NaN as
    // peers cannot be checked here (bits would keep the zeros apart and every NaN payload to itself); Boolean keys are bit-packed and Utf8
    // keys have no fixed width — dictionary-encode strings first (dfgpu_table_dictionary_encode).
    DFGPU_CHECK(c.field.type != DFGPU_FLOAT64, "Float64 window keys are not supported on the GPU path");
    DFGPU_CHECK(c.field.type != DFGPU_BOOL, "Boolean window keys are not supported on the GPU path");
    DFGPU_CHECK(c.field.type != DFGPU_UTF8, "Utf8 window keys are not supported on the GPU path");
    ks.c[k] = KeyCol{c.ptr(), c.valid_words(), c.field.type, type_width(c.field.type)};
  }
  return ks;
}

static Table window_table(const Table& in, const int* partition_cols, int n_partition, const int* order_cols, int n_order, const dfgpu_window_spec* specs, int n_specs) {
  Runtime& r = rt();
  const int64_t n = in.nrows;
  const int64_t n_words = (n + 63) / 64;
  DFGPU_CHECK(n_specs >= 0 && (n_specs == 0 || specs != nullptr), "window expressions missing");
  const KeySet part = window_keys(in, partition_cols, n_partition), order = window_keys(in, order_cols, n_order);
  for (int s = 0; s < n_specs; s++) {   // an unknown function or a bad parameter is an error before anything runs
    const dfgpu_window_spec& spec = specs[s];
    const char* fn = win_func_name(spec.func);
    DFGPU_CHECK(spec.func != DFGPU_WINDOW_NTILE || spec.n >= 1, "NTILE needs a positive number of buckets");
    if (spec.func == DFGPU_WINDOW_FIRST_VALUE || spec.func == DFGPU_WINDOW_LAST_VALUE || spec.func == DFGPU_WINDOW_NTH_VALUE) {
      DFGPU_CHECK(spec.has_arg != 0, std::string(fn) + " needs an argument");
      DFGPU_CHECK(spec.func != DFGPU_WINDOW_NTH_VALUE || spec.n != 0, "NTH_VALUE needs a non-zero n");
      DFGPU_CHECK(spec.frame == DFGPU_WINDOW_RANGE_TO_CURRENT || spec.frame == DFGPU_WINDOW_ROWS_TO_CURRENT || spec.frame == DFGPU_WINDOW_PARTITION,
                  "unknown dfgpu_window_frame " + std::to_string(spec.frame));
    }
  }
  Table out;
  out.device = in.device;
  out.nrows = n;
  out.cols = in.cols;   // the same buffers
  if (n_specs == 0) return out;

  BufPtr part_heads, peer_heads;
  if (n > 0) {
    part_heads = make_buf((size_t)n_words * 8);
    peer_heads = make_buf((size_t)n_words * 8);
    int64_t key_bytes = 0;
    for (int k = 0; k < part.n; k++) key_bytes += part.c[k].width;
    for (int k = 0; k < order.n; k++) key_bytes += order.c[k].width;
    ProfileScope ps("window_heads", n * key_bytes + n_words * 16);
    k_window_heads<<<grid_for(n_words, BLOCK / WAVE), BLOCK, 0, r.stream>>>(part, order, n, part_heads->as<uint64_t>(), peer_heads->as<uint64_t>());
    DFGPU_HIP(hipGetLastError());
  }
  // positions, made when the first function asks: starts by a forward max scan, ends by a min scan over the rows in reverse
  BufPtr part_start, peer_start, part_end, peer_end;
  const auto positions = [&](BufPtr& slot, const BufPtr& heads, bool end) -> const int64_t* {
    if (!slot) {
      slot = make_buf((size_t)n * 8);
      WinIn pin{nullptr, nullptr, nullptr, heads->as<uint64_t>(), n, end ? WS_END_POS : WS_START_POS, end ? 1 : 0};
      if (end) run_window_scan<OpMinI64>(pin, slot->ptr, nullptr, "window_ends", n / 8 + n * 8);
      else run_window_scan<OpMaxI64>(pin, slot->ptr, nullptr, "window_starts", n / 8 + n * 8);
    }
    return slot->as<int64_t>();
  };
  // the same per 64-row word (PERCENT_RANK .. NTH_VALUE): made when the first function asks, once per bitmap and direction
  BufPtr part_word_start, peer_word_start, part_word_end, peer_word_end;
  const auto word_positions = [&](BufPtr& slot, const BufPtr& heads, bool end) -> const int64_t* {
    if (!slot) {
      slot = make_buf((size_t)n_words * 8);
      WinIn pin{nullptr, nullptr, nullptr, heads->as<uint64_t>(), n_words, end ? WS_WORD_END : WS_WORD_START, end ? 1 : 0, n};
      if (end) run_window_scan<OpMinI64>(pin, slot->ptr, nullptr, "window_word_ends", n_words * 16);
      else run_window_scan<OpMaxI64>(pin, slot->ptr, nullptr, "window_word_starts", n_words * 16);
    }
    return slot->as<int64_t>();
  };
  const auto part_words = [&](bool starts, bool ends) {
    return WinWords{part_heads->as<uint64_t>(), starts ? word_positions(part_word_start, part_heads, false) : nullptr,
                    ends ? word_positions(part_word_end, part_heads, true) : nullptr};
  };
  const auto peer_words = [&](bool starts, bool ends) {
    return WinWords{peer_heads->as<uint64_t>(), starts ? word_positions(peer_word_start, peer_heads, false) : nullptr,
                    ends ? word_positions(peer_word_end, peer_heads, true) : nullptr};
  };
  int peers_unique = -1;   // every peer group is one row: RANGE frames are ROWS frames (asked once, by the first RANGE frame)
  const auto all_peers_unique = [&]() {
    if (peers_unique < 0) {
      BufPtr total = make_zero_buf(8);
      {
        ProfileScope ps("window_peer_popcount", n_words * 8);
        k_window_popcount<<<grid_for(n_words, BLOCK), BLOCK, 0, r.stream>>>(peer_heads->as<uint64_t>(), n_words, total->as<unsigned long long>());
        DFGPU_HIP(hipGetLastError());
      }
      peers_unique = (int64_t)read_u64(total->as<uint64_t>()) == n ? 1 : 0;
    }
    return peers_unique == 1;
  };

  for (int s = 0; s < n_specs; s++) {
    const dfgpu_window_spec& spec = specs[s];
    const std::string name = spec.name ? spec.name : "";
    const int func = spec.func;
    if (func == DFGPU_WINDOW_PERCENT_RANK || func == DFGPU_WINDOW_CUME_DIST || func == DFGPU_WINDOW_NTILE) {
      const bool ntile = func == DFGPU_WINDOW_NTILE;
      Column c = alloc_column(wfld(ntile ? DFGPU_UINT64 : DFGPU_FLOAT64, 0, 0, 0), name, n);
      c.null_count = 0;
      if (n > 0) {
        const WinWords pw = part_words(true, true);
        const WinWords ow = ntile ? WinWords{nullptr, nullptr, nullptr} : peer_words(func == DFGPU_WINDOW_PERCENT_RANK, func == DFGPU_WINDOW_CUME_DIST);
        ProfileScope ps("window_dist", n * 8 + n_words * (ntile ? 24 : 40));   // the result; per word a bitmap and two summaries, and the peers' two
        k_window_dist<<<grid_for(n_words, BLOCK / WAVE), BLOCK, 0, r.stream>>>(ntile ? WD_NTILE : func == DFGPU_WINDOW_PERCENT_RANK ? WD_PERCENT_RANK : WD_CUME_DIST, pw, ow,
                                                                            (uint64_t)spec.n, n, c.data->ptr);
        DFGPU_HIP(hipGetLastError());
      }
      out.cols.push_back(std::move(c));
      continue;
    }
    if (func == DFGPU_WINDOW_FIRST_VALUE || func == DFGPU_WINDOW_LAST_VALUE || func == DFGPU_WINDOW_NTH_VALUE) {
      Column arg = datum_to_column(evaluate(spec.arg, in), n, name);
      DFGPU_CHECK(arg.dict || (arg.field.type != DFGPU_BOOL && arg.field.type != DFGPU_UTF8),
                  std::string(win_func_name(func)) + "(" + name + ") over " + win_type_name(arg) + " is not supported on the GPU path");
      const int width = type_width(arg.field.type);
      dfgpu_field of = arg.field;
      of.nullable = 1;
      if (func == DFGPU_WINDOW_LAST_VALUE && spec.frame == DFGPU_WINDOW_ROWS_TO_CURRENT) {   // the argument itself: no launch
        arg.field = of;
        arg.name = name;
        if (arg.null_count < 0) count_nulls(arg);
        out.cols.push_back(std::move(arg));
        continue;
      }
      Column c = alloc_column(of, name, n, n > 0);
      c.dict = arg.dict;
      if (n == 0) {
        c.null_count = 0;
        out.cols.push_back(std::move(c));
        continue;
      }
      const int pick = func == DFGPU_WINDOW_FIRST_VALUE ? WP_FIRST : func == DFGPU_WINDOW_LAST_VALUE ? WP_LAST : WP_NTH;
      const WinWords pw = pick != WP_LAST ? part_words(true, false) : WinWords{nullptr, nullptr, nullptr};
      WinWords fw{nullptr, nullptr, nullptr};
      if (pick != WP_FIRST && spec.frame == DFGPU_WINDOW_PARTITION) fw = part_words(false, true);
      else if (pick != WP_FIRST && spec.frame == DFGPU_WINDOW_RANGE_TO_CURRENT) fw = peer_words(false, true);
      {
        // the argument and its validity once, the result and its validity once, per word a bitmap and a summary for each end that is read
        ProfileScope ps("window_value", n * 2 * width + (arg.validity ? n / 8 : 0) + n / 8 + n_words * 16 * ((pw.heads ? 1 : 0) + (fw.heads ? 1 : 0)));
        const int g = grid_for(n_words, BLOCK / WAVE);
        uint64_t* ov = c.validity->as<uint64_t>();
        switch (width) {
          case 1: k_window_value<1><<<g, BLOCK, 0, r.stream>>>(pick, spec.n, pw, fw, arg.ptr(), arg.valid_words(), n, c.data->ptr, ov); break;
          case 4: k_window_value<4><<<g, BLOCK, 0, r.stream>>>(pick, spec.n, pw, fw, arg.ptr(), arg.valid_words(), n, c.data->ptr, ov); break;
          case 8: k_window_value<8><<<g, BLOCK, 0, r.stream>>>(pick, spec.n, pw, fw, arg.ptr(), arg.valid_words(), n, c.data->ptr, ov); break;
          case 16: k_window_value<16><<<g, BLOCK, 0, r.stream>>>(pick, spec.n, pw, fw, arg.ptr(), arg.valid_words(), n, c.data->ptr, ov); break;
          default: throw Error("window value function over a column of " + std::to_string(width) + " bytes per value");
        }
        DFGPU_HIP(hipGetLastError());
      }
      count_nulls(c);
      out.cols.push_back(std::move(c));
      continue;
    }
    if (func == DFGPU_WINDOW_ROW_NUMBER || func == DFGPU_WINDOW_RANK || func == DFGPU_WINDOW_DENSE_RANK) {
      Column c = alloc_column(wfld(DFGPU_UINT64, 0, 0, 0), name, n);
      c.null_count = 0;
      if (n > 0 && func == DFGPU_WINDOW_DENSE_RANK) {
        WinIn din{nullptr, nullptr, part_heads->as<uint64_t>(), peer_heads->as<uint64_t>(), n, WS_BIT, 0};
        run_window_scan<OpAddU64>(din, c.data->ptr, nullptr, "window_dense_rank", n / 4 + n * 8);
      } else if (n > 0) {
        const int64_t* ps_ = positions(part_start, part_heads, false);
        const int64_t* pe_ = func == DFGPU_WINDOW_RANK ? positions(peer_start, peer_heads, false) : nullptr;
        ProfileScope ps("window_rank", n * (func == DFGPU_WINDOW_RANK ? 24 : 16));
        k_window_rank<<<grid_for(n, BLOCK), BLOCK, 0, r.stream>>>(func == DFGPU_WINDOW_RANK ? 1 : 0, ps_, pe_, n, c.data->as<uint64_t>());
        DFGPU_HIP(hipGetLastError());
      }
      out.cols.push_back(std::move(c));
      continue;
    }
    DFGPU_CHECK(spec.frame == DFGPU_WINDOW_RANGE_TO_CURRENT || spec.frame == DFGPU_WINDOW_ROWS_TO_CURRENT || spec.frame == DFGPU_WINDOW_PARTITION,
                "unknown dfgpu_window_frame " + std::to_string(spec.frame));
    Column arg;
    const bool has_arg = spec.has_arg != 0;
    DFGPU_CHECK(has_arg || func == DFGPU_WINDOW_COUNT, std::string(win_func_name(func)) + " needs an argument");
    if (has_arg) arg = datum_to_column(evaluate(spec.arg, in), n, name);
    const WinPlan p = plan_window(func, has_arg ? &arg : nullptr);
    const bool nullable = p.fin != WF_COUNT;
    Column c = alloc_column(p.out, name, n, nullable && n > 0);
    if (n == 0) {
      c.null_count = 0;
      out.cols.push_back(std::move(c));
      continue;
    }
    const int in_width = !has_arg || p.src == WS_NONE ? 0 : type_width(arg.field.type);
    BufPtr sv = make_buf((size_t)n * p.velem), sc = make_buf((size_t)n * 8);
    WinIn win{has_arg ? arg.ptr() : nullptr, has_arg ? arg.valid_words() : nullptr, part_heads->as<uint64_t>(), nullptr, n, p.src, 0};
    run_window_op(p.op, win, sv->ptr, sc->as<uint64_t>(), n * (in_width + p.velem + 8) + (win.valid ? n / 8 : 0) + n / 8);
    const int64_t* pos = nullptr;
    if (spec.frame == DFGPU_WINDOW_PARTITION) pos = positions(part_end, part_heads, true);
    else if (spec.frame == DFGPU_WINDOW_RANGE_TO_CURRENT && !all_peers_unique()) pos = positions(peer_end, peer_heads, true);
    BufPtr overflow = p.fin == WF_AVG_DEC ? make_zero_buf(4) : nullptr;
    const int out_width = type_width(p.out.type);
    {
      ProfileScope ps(pos ? "window_pick" : "window_finish", n * (p.velem + 8 + out_width + (pos ? 8 : 0)) + n / 8);
      const int g = grid_for(n_words, BLOCK / WAVE);
      uint64_t* ov = c.validity ? c.validity->as<uint64_t>() : nullptr;
      int* of = overflow ? overflow->as<int>() : nullptr;
      if (pos) k_window_finish<true><<<g, BLOCK, 0, r.stream>>>(sv->ptr, sc->as<uint64_t>(), pos, p.fin, p.mul, n, c.data->ptr, ov, of);
      else k_window_finish<false><<<g, BLOCK, 0, r.stream>>>(sv->ptr, sc->as<uint64_t>(), nullptr, p.fin, p.mul, n, c.data->ptr, ov, of);
      DFGPU_HIP(hipGetLastError());
    }
    if (overflow) {
      int bad = 0;
      d2h(&bad, overflow->ptr, 4);
      DFGPU_CHECK(!bad, "AVG(" + name + "): the Decimal128 sum scaled to the result's scale overflows 128 bits");
    }
    if (nullable) count_nulls(c);
    else c.null_count = 0;
    out.cols.push_back(std::move(c));
  }
  return out;
}

}  // namespace dfgpu

using namespace dfgpu;

extern "C" int dfgpu_window(dfgpu_table_t input, const int* partition_cols, int n_partition, const int* order_cols, int n_order, const dfgpu_window_spec* specs,
                            int n_specs, dfgpu_table_t* out) {
  return guarded([&] {
    require_init();
    const Table& in = *unwrap(input);
    auto t = std::make_unique<Table>(window_table(in, partition_cols, n_partition, order_cols, n_order, specs, n_specs));
    *out = wrap(t.release());
  });
}
