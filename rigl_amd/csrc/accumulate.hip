// Micro-batch gradient accumulation: one streaming pass over the whole gradient arena per micro-batch, plus the loss scalar
// on one lane of the same launch.
//   FIRST : acc = g           loss_acc = loss                       (a copy: a stale acc can never leak into a step)
//   ADD   : acc = acc + g     loss_acc = loss_acc + loss
//   LAST  : g   = acc + g     loss_mean = (loss_acc + loss) * inv_k  (acc and loss_acc are only read)
// HBM-bound: 16 B per lane, UNROLL independent loads per operand in flight before the first use, grid capped at 8 blocks
// per CU with a grid-stride loop over whole tiles.  Each element is one fp32 addition whose operands depend on the element
// index alone, so the result bits do not depend on the grid.
// rigl_grad_accumulate_ranges is the same pass over up to RIGL_ACC_MAX_RANGES ranges of the arenas in one launch: what a
// data-parallel step needs of LAST, bucket by bucket in front of each bucket's all-reduce (see k_accumulate_ranges below).
#include "common.hpp"

// One IEEE fp32 addition per element, and the loss mean's addition and product rounded separately (no FMA).
#pragma clang fp contract(off)

namespace rigl {
namespace kacc {

constexpr int BLOCK = 256;
constexpr int UNROLL = 4;                                  // float4 per lane and operand in flight
constexpr int64_t TILE_QUADS = (int64_t)BLOCK * UNROLL;    // float4 per block and iteration (4096 elements)
constexpr int DEFAULT_MAX_BLOCKS = 2048;                   // 256 CUs x 8 blocks

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
  return make_float4(__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w));
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_accumulate(int64_t n, float* __restrict__ acc, float* __restrict__ grad,
                                                      const float* __restrict__ loss, float* __restrict__ loss_acc,
                                                      float* __restrict__ loss_mean, float inv_k) {
  // FIRST reads grad and writes acc; ADD reads both and writes acc; LAST reads both and writes grad.  An element is read and
  // written by the same lane in the same iteration, so writing one operand in place is safe.
  float* const dst = MODE == RIGL_ACC_LAST ? grad : acc;
  const int64_t nq = n >> 2;                               // full quads
  const int64_t n_tiles = nq / TILE_QUADS;                 // whole tiles: no bounds checks, all loads issued before the adds
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t q0 = t * TILE_QUADS + threadIdx.x;
    float4 g[UNROLL], a[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) g[u] = reinterpret_cast<const float4*>(grad)[q0 + u * BLOCK];
    if (MODE != RIGL_ACC_FIRST) {
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) a[u] = reinterpret_cast<const float4*>(acc)[q0 + u * BLOCK];
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u)
      reinterpret_cast<float4*>(dst)[q0 + u * BLOCK] = MODE == RIGL_ACC_FIRST ? g[u] : add4(a[u], g[u]);
  }
  if (blockIdx.x != 0) return;
  // the quads behind the last whole tile (fewer than TILE_QUADS), then the n % 4 elements behind the last quad
  for (int64_t q = n_tiles * TILE_QUADS + threadIdx.x; q < nq; q += BLOCK) {
    const float4 g = reinterpret_cast<const float4*>(grad)[q];
    if (MODE == RIGL_ACC_FIRST) reinterpret_cast<float4*>(dst)[q] = g;
    else reinterpret_cast<float4*>(dst)[q] = add4(reinterpret_cast<const float4*>(acc)[q], g);
  }
  const int64_t e = (nq << 2) + threadIdx.x;
  if (e < n) dst[e] = MODE == RIGL_ACC_FIRST ? grad[e] : __fadd_rn(acc[e], grad[e]);
  if (loss != nullptr && threadIdx.x == BLOCK - 1) {
    const float l = *loss;
    if (MODE == RIGL_ACC_FIRST) *loss_acc = l;
    else if (MODE == RIGL_ACC_ADD) *loss_acc = __fadd_rn(*loss_acc, l);
    else *loss_mean = __fmul_rn(__fadd_rn(*loss_acc, l), inv_k);
  }
}

// ---- the same pass over a table of ranges (rigl_grad_accumulate_ranges) --------------------------------------------------------
// The ranges, each rounded up to whole quads, are laid end to end and that concatenation is cut into tiles of TILE_QUADS, so
// every tile but the last is full whatever the ranges' lengths.  A tile that lies in the full quads of ONE range -- all but
// at most two per range -- is the tile of k_accumulate: no bounds checks, every load issued before the first add.  A tile that
// meets a range's end looks its range up per quad and moves the range's last length % 4 elements one by one.  An element's
// operands depend on its index alone, so the bits depend neither on the grid nor on how the elements are cut into ranges.
constexpr int MAX_RANGES = RIGL_ACC_MAX_RANGES;

struct Ranges {
  int64_t off[MAX_RANGES];    // first element of range i (a multiple of 4)
  int64_t len[MAX_RANGES];    // its elements
  int64_t quad0[MAX_RANGES];  // its first quad in the concatenation
  int64_t total;              // quads of the concatenation
  int32_t n;
};
static_assert(sizeof(Ranges) <= 4096, "the by-value table must fit the kernel arguments");

// The range that holds quad q < total of the concatenation: the last one that starts at or before q (an empty range shares its
// start with its successor, or with `total` when none follows, so it is never that one).  Constant indices only: the table is
// read from the kernel arguments, never copied to scratch.
__device__ __forceinline__ void find_range(const Ranges& R, int64_t q, int64_t& off, int64_t& len, int64_t& quad0) {
  off = R.off[0];
  len = R.len[0];
  quad0 = R.quad0[0];
#pragma unroll
  for (int i = 1; i < MAX_RANGES; ++i) {
    if (i < R.n && R.quad0[i] <= q) {
      off = R.off[i];
      len = R.len[i];
      quad0 = R.quad0[i];
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void k_accumulate_ranges(Ranges R, float* __restrict__ acc, float* __restrict__ grad,
                                                             const float* __restrict__ loss, float* __restrict__ loss_acc,
                                                             float* __restrict__ loss_mean, float inv_k) {
  float* const dst = MODE == RIGL_ACC_LAST ? grad : acc;
  const int64_t n_tiles = (R.total + TILE_QUADS - 1) / TILE_QUADS;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t tq = t * TILE_QUADS;                     // the tile's first quad in the concatenation
    int64_t off, len, quad0;
    find_range(R, tq, off, len, quad0);
    if (tq + TILE_QUADS <= quad0 + (len >> 2)) {           // inside the full quads of one range: the tile of k_accumulate
      const int64_t q0 = (off >> 2) + (tq - quad0) + threadIdx.x;
      float4 g[UNROLL], a[UNROLL];
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) g[u] = reinterpret_cast<const float4*>(grad)[q0 + u * BLOCK];
      if (MODE != RIGL_ACC_FIRST) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) a[u] = reinterpret_cast<const float4*>(acc)[q0 + u * BLOCK];
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u)
        reinterpret_cast<float4*>(dst)[q0 + u * BLOCK] = MODE == RIGL_ACC_FIRST ? g[u] : add4(a[u], g[u]);
      continue;
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {                     // a tile that meets the end of a range (or of the table)
      const int64_t q = tq + u * BLOCK + threadIdx.x;
      if (q < R.total) {
        find_range(R, q, off, len, quad0);
        const int64_t e = off + ((q - quad0) << 2);        // the quad's first element, and how many the range has from there
        const int64_t left = off + len - e;                // >= 1: a range has ceil(len / 4) quads
        if (left >= 4) {
          const float4 gq = *reinterpret_cast<const float4*>(grad + e);
          if (MODE == RIGL_ACC_FIRST) *reinterpret_cast<float4*>(dst + e) = gq;
          else *reinterpret_cast<float4*>(dst + e) = add4(*reinterpret_cast<const float4*>(acc + e), gq);
        } else {
          for (int64_t j = e; j < e + left; ++j) dst[j] = MODE == RIGL_ACC_FIRST ? grad[j] : __fadd_rn(acc[j], grad[j]);
        }
      }
    }
  }
  if (blockIdx.x == 0 && loss != nullptr && threadIdx.x == BLOCK - 1) {   // once per launch, whatever the table holds
    const float l = *loss;
    if (MODE == RIGL_ACC_FIRST) *loss_acc = l;
    else if (MODE == RIGL_ACC_ADD) *loss_acc = __fadd_rn(*loss_acc, l);
    else *loss_mean = __fmul_rn(__fadd_rn(*loss_acc, l), inv_k);
  }
}

}  // namespace kacc
}  // namespace rigl

extern "C" {

int rigl_grad_accumulate(int64_t n, float* acc, float* grad, int32_t mode, const float* loss, float* loss_acc,
                         float* loss_mean, float inv_k, int32_t max_blocks, rigl_stream_t stream) {
  using namespace rigl;
  if (n < 0) return fail(RIGL_EINVAL, "rigl_grad_accumulate: n = %lld < 0", (long long)n);
  if (!acc || !grad || acc == grad) return fail(RIGL_EINVAL, "rigl_grad_accumulate: acc / grad NULL or the same buffer");
  if (((uintptr_t)acc | (uintptr_t)grad) & 15u) return fail(RIGL_EINVAL, "rigl_grad_accumulate: acc / grad not 16-byte aligned");
  if (mode != RIGL_ACC_FIRST && mode != RIGL_ACC_ADD && mode != RIGL_ACC_LAST)
    return fail(RIGL_EINVAL, "rigl_grad_accumulate: unknown mode %d", mode);
  if (max_blocks < 0) return fail(RIGL_EINVAL, "rigl_grad_accumulate: max_blocks = %d < 0", max_blocks);
  if (loss) {
    if (!loss_acc) return fail(RIGL_EINVAL, "rigl_grad_accumulate: loss without loss_acc");
    if (mode == RIGL_ACC_LAST && !loss_mean) return fail(RIGL_EINVAL, "rigl_grad_accumulate: LAST with a loss needs loss_mean");
    if (((uintptr_t)loss | (uintptr_t)loss_acc | (mode == RIGL_ACC_LAST ? (uintptr_t)loss_mean : 0)) & 3u)
      return fail(RIGL_EINVAL, "rigl_grad_accumulate: loss / loss_acc / loss_mean not 4-byte aligned");
  }
  if (n == 0 && !loss) return RIGL_OK;
  const int64_t cap = max_blocks > 0 ? max_blocks : kacc::DEFAULT_MAX_BLOCKS;
  int64_t blocks = (n >> 2) / kacc::TILE_QUADS;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const dim3 g((unsigned)blocks), b(kacc::BLOCK);
  hipStream_t s = as_stream(stream);
  switch (mode) {
    case RIGL_ACC_FIRST:
      hipLaunchKernelGGL((kacc::k_accumulate<RIGL_ACC_FIRST>), g, b, 0, s, n, acc, grad, loss, loss_acc, loss_mean, inv_k);
      break;
    case RIGL_ACC_ADD:
      hipLaunchKernelGGL((kacc::k_accumulate<RIGL_ACC_ADD>), g, b, 0, s, n, acc, grad, loss, loss_acc, loss_mean, inv_k);
      break;
    default:
      hipLaunchKernelGGL((kacc::k_accumulate<RIGL_ACC_LAST>), g, b, 0, s, n, acc, grad, loss, loss_acc, loss_mean, inv_k);
      break;
  }
  RIGL_CHECK_LAUNCH("rigl_grad_accumulate");
  return RIGL_OK;
}

int rigl_grad_accumulate_ranges(int64_t n, float* acc, float* grad, const RiglAccRange* ranges, int32_t n_ranges, int32_t mode,
                                const float* loss, float* loss_acc, float* loss_mean, float inv_k, int32_t max_blocks,
                                rigl_stream_t stream) {
  using namespace rigl;
  const char* who = "rigl_grad_accumulate_ranges";
  if (n < 0) return fail(RIGL_EINVAL, "%s: n = %lld < 0", who, (long long)n);
  if (!acc || !grad || acc == grad) return fail(RIGL_EINVAL, "%s: acc / grad NULL or the same buffer", who);
  if (((uintptr_t)acc | (uintptr_t)grad) & 15u) return fail(RIGL_EINVAL, "%s: acc / grad not 16-byte aligned", who);
  if (mode != RIGL_ACC_FIRST && mode != RIGL_ACC_ADD && mode != RIGL_ACC_LAST)
    return fail(RIGL_EINVAL, "%s: unknown mode %d", who, mode);
  if (max_blocks < 0) return fail(RIGL_EINVAL, "%s: max_blocks = %d < 0", who, max_blocks);
  if (loss) {
    if (!loss_acc) return fail(RIGL_EINVAL, "%s: loss without loss_acc", who);
    if (mode == RIGL_ACC_LAST && !loss_mean) return fail(RIGL_EINVAL, "%s: LAST with a loss needs loss_mean", who);
    if (((uintptr_t)loss | (uintptr_t)loss_acc | (mode == RIGL_ACC_LAST ? (uintptr_t)loss_mean : 0)) & 3u)
      return fail(RIGL_EINVAL, "%s: loss / loss_acc / loss_mean not 4-byte aligned", who);
  }
  if (n_ranges < 0 || n_ranges > kacc::MAX_RANGES)
    return fail(RIGL_EINVAL, "%s: %d ranges (0 .. %d)", who, n_ranges, kacc::MAX_RANGES);
  if (n_ranges > 0 && !ranges) return fail(RIGL_EINVAL, "%s: NULL table", who);
  kacc::Ranges R;
  R.n = n_ranges;
  R.total = 0;
  int64_t end = 0;                                         // one past the range in front
  for (int32_t i = 0; i < kacc::MAX_RANGES; ++i) {
    R.off[i] = R.len[i] = 0;
    R.quad0[i] = R.total;
    if (i >= n_ranges) continue;
    const int64_t o = ranges[i].offset, l = ranges[i].length;
    if (o < 0 || l < 0) return fail(RIGL_EINVAL, "%s: range %d: offset %lld, length %lld", who, i, (long long)o, (long long)l);
    if (o & 3) return fail(RIGL_EINVAL, "%s: range %d: offset %lld is no multiple of 4", who, i, (long long)o);
    if (o > n || l > n - o)
      return fail(RIGL_EINVAL, "%s: range %d: [%lld, +%lld) ends beyond n = %lld", who, i, (long long)o, (long long)l, (long long)n);
    if (o < end) return fail(RIGL_EINVAL, "%s: range %d starts at %lld, inside or in front of range %d", who, i, (long long)o, i - 1);
    end = o + l;
    R.off[i] = o;
    R.len[i] = l;
    R.total += (l + 3) >> 2;
  }
  if (R.total == 0 && !loss) return RIGL_OK;
  const int64_t cap = max_blocks > 0 ? max_blocks : kacc::DEFAULT_MAX_BLOCKS;
  int64_t blocks = (R.total + kacc::TILE_QUADS - 1) / kacc::TILE_QUADS;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const dim3 g((unsigned)blocks), b(kacc::BLOCK);
  hipStream_t s = as_stream(stream);
  switch (mode) {
    case RIGL_ACC_FIRST:
      hipLaunchKernelGGL((kacc::k_accumulate_ranges<RIGL_ACC_FIRST>), g, b, 0, s, R, acc, grad, loss, loss_acc, loss_mean, inv_k);
      break;
    case RIGL_ACC_ADD:
      hipLaunchKernelGGL((kacc::k_accumulate_ranges<RIGL_ACC_ADD>), g, b, 0, s, R, acc, grad, loss, loss_acc, loss_mean, inv_k);
      break;
    default:
      hipLaunchKernelGGL((kacc::k_accumulate_ranges<RIGL_ACC_LAST>), g, b, 0, s, R, acc, grad, loss, loss_acc, loss_mean, inv_k);
      break;
  }
  RIGL_CHECK_LAUNCH(who);
  return RIGL_OK;
}

}  // extern "C"
