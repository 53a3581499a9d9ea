// Training-state snapshots: a table of device regions <-> one packed device image, at copy rate, with a per-region digest.
//   rigl_state_gather  : regions -> packed (zero padding behind every region), digests of the words read
//   rigl_state_scatter : packed -> regions (the padding is never read),        digests of the words written
// One copy launch per RIGL_STATE_BATCH regions (the table by value), then ONE finalize launch.  A region is cut into chunks of
// RIGL_STATE_CHUNK words; a workgroup moves a chunk 16 B per lane with UNROLL loads in flight (accumulate.hip's pass) and leaves
// the chunk's two partial sums; the finalize launch adds a region's partials and writes its digest, so every call writes every
// digest and reads nothing the buffer held before.  The sums are integers mod 2^64: associative and commutative, so the bits do
// not depend on the grid or on the order of the partials.  No atomics, plain vector loads and stores.
//
// The packed side of a chunk is 16-B aligned by construction (256-B region offsets, 64 KiB chunks).  Where the region pointer is
// 16-B aligned too, both sides move as 16-B accesses; a region pointer that is only 4-B aligned keeps the 16-B accesses on the
// packed side and takes four 4-B accesses per quad on its own.  The bytes % 16 tail is moved word by word.
// (That path is for correctness: no tensor of a training state is misaligned, and its rate was not measured.)
// The table travels in the kernel arguments and is indexed dynamically (the binary search over chunk0, r[lo]); the compiler
// serves that from the kernarg segment with scalar loads, not from scratch: all three kernels have a private segment of 0
// bytes (hipcc -S, .private_segment_fixed_size).
#include "common.hpp"

namespace rigl {
namespace kstate {

constexpr int BLOCK = 256;
constexpr int UNROLL = 4;                         // uint4 per lane in flight
constexpr int CHUNK = RIGL_STATE_CHUNK;           // words per chunk
constexpr int BATCH = RIGL_STATE_BATCH;           // regions per copy launch
constexpr int64_t ALIGN = RIGL_STATE_ALIGN;       // bytes: a region's offset in the packed image
constexpr int DEFAULT_MAX_BLOCKS = 2048;          // 256 CUs x 8 blocks
constexpr int FIN_BLOCK = 1024;                   // the finalize: one workgroup of sixteen waves per region

static_assert(CHUNK % (4 * BLOCK * UNROLL) == 0, "a chunk is whole tiles");
static_assert((CHUNK * 4) % ALIGN == 0, "chunks start on the packed side's alignment");
static_assert(CHUNK <= (1 << 16), "the chunk-local index times a word stays inside one 32 x 32 -> 64 bit product");

struct Reg {
  uint32_t* ptr;        // the region
  int64_t words;        // bytes / 4
  int64_t packed_word;  // its first word in the packed image
};

struct Batch {
  Reg r[BATCH];
  int32_t chunk0[BATCH + 1];  // first chunk of region i inside this batch; [n] = the batch's chunk count
  int32_t n;                  // regions in this batch
  int32_t first_region;       // index of r[0] in the caller's table
  int32_t chunk_base;         // chunks of the batches in front
};

struct Part { uint64_t s1, s2; };   // one chunk: sum w, sum (i + 1) * w with i the word's index in its REGION

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int off) {
  const uint32_t lo = __shfl_down((uint32_t)v, off, 64), hi = __shfl_down((uint32_t)(v >> 32), off, 64);
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ void wave_sum(uint64_t& a, uint64_t& b) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += shfl_down_u64(a, off);
    b += shfl_down_u64(b, off);
  }
}

// t1 += the quad's words, t2 += (j + 1) * word for the chunk-local indices j = j0 .. j0 + 3 (j0 + 4 <= CHUNK <= 2^16)
__device__ __forceinline__ void digest4(uint64_t& t1, uint64_t& t2, uint4 v, uint32_t j0) {
  t1 += (uint64_t)v.x + v.y + v.z + v.w;
  t2 += (uint64_t)(j0 + 1u) * v.x + (uint64_t)(j0 + 2u) * v.y + (uint64_t)(j0 + 3u) * v.z + (uint64_t)(j0 + 4u) * v.w;
}

template <bool VEC>
__device__ __forceinline__ uint4 load4(const uint32_t* p) {
  if (VEC) return *reinterpret_cast<const uint4*>(p);
  return make_uint4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ __forceinline__ void store4(uint32_t* p, uint4 v) {
  if (VEC) { *reinterpret_cast<uint4*>(p) = v; return; }
  p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}

// Moves the m words of one chunk from src to dst (SRC_VEC / DST_VEC: that side is 16-B aligned) and digests them.
template <bool SRC_VEC, bool DST_VEC>
__device__ __forceinline__ void move_chunk(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int m, uint64_t& t1,
                                           uint64_t& t2) {
  const int nq = m >> 2;
  int q = threadIdx.x;
  for (; q + (UNROLL - 1) * BLOCK < nq; q += UNROLL * BLOCK) {   // whole tiles: all loads issued before the first use
    uint4 v[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) v[u] = load4<SRC_VEC>(src + ((q + u * BLOCK) << 2));
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      store4<DST_VEC>(dst + ((q + u * BLOCK) << 2), v[u]);
      digest4(t1, t2, v[u], (uint32_t)((q + u * BLOCK) << 2));
    }
  }
  for (; q < nq; q += BLOCK) {                                   // the quads behind the last whole tile
    const uint4 v = load4<SRC_VEC>(src + (q << 2));
    store4<DST_VEC>(dst + (q << 2), v);
    digest4(t1, t2, v, (uint32_t)(q << 2));
  }
  if ((int)threadIdx.x < (m & 3)) {                              // the m % 4 words behind the last quad
    const int j = (nq << 2) + threadIdx.x;
    const uint32_t w = src[j];
    dst[j] = w;
    t1 += w;
    t2 += (uint64_t)(uint32_t)(j + 1) * w;
  }
}

template <bool GATHER>
__global__ __launch_bounds__(BLOCK) void k_move(Batch B, uint32_t* __restrict__ packed, Part* __restrict__ parts,
                                                int32_t* __restrict__ region_chunk0) {
  __shared__ uint64_t sh[BLOCK / 64][2];
  // the chunk range of every region of this batch, for the finalize launch (index first_region + n is written again, with the
  // same value, by the next batch)
  if (blockIdx.x == 0 && (int)threadIdx.x <= B.n) region_chunk0[B.first_region + threadIdx.x] = B.chunk_base + B.chunk0[threadIdx.x];
  const int total = B.chunk0[B.n];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = B.n - 1;                    // the last region whose first chunk is <= c (empty regions share a start: skipped)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (B.chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const Reg R = B.r[lo];
    const int64_t base = (int64_t)(c - B.chunk0[lo]) * CHUNK;    // first word of this chunk in its region
    const int64_t left = R.words - base;
    const int m = left < CHUNK ? (int)left : CHUNK;              // words [base, base + m) inside [0, words)
    uint32_t* reg = R.ptr + base;
    uint32_t* pk = packed + R.packed_word + base;
    const bool vec = (reinterpret_cast<uintptr_t>(R.ptr) & 15u) == 0;   // (base * 4 is a multiple of 16)
    uint64_t t1 = 0, t2 = 0;
    if (GATHER) {
      if (vec) move_chunk<true, true>(reg, pk, m, t1, t2);
      else move_chunk<false, true>(reg, pk, m, t1, t2);
      if (left <= CHUNK) {                                       // the region's last chunk: zero words up to the next region's start
        const int pad = (int)(((R.words + 63) & ~(int64_t)63) - R.words);
        if ((int)threadIdx.x < pad) pk[m + threadIdx.x] = 0u;
      }
    } else {
      if (vec) move_chunk<true, true>(pk, reg, m, t1, t2);
      else move_chunk<true, false>(pk, reg, m, t1, t2);
    }
    wave_sum(t1, t2);
    if (lane == 0) { sh[wave][0] = t1; sh[wave][1] = t2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      Part p = {sh[0][0], sh[0][1]};
#pragma unroll
      for (int v = 1; v < BLOCK / 64; ++v) { p.s1 += sh[v][0]; p.s2 += sh[v][1]; }
      p.s2 += (uint64_t)base * p.s1;                             // chunk-local indices -> the region's
      parts[B.chunk_base + c] = p;
    }
    __syncthreads();                                             // sh is reused by the next chunk
  }
}

// One workgroup per region: its chunk partials lane-strided (a 100 MB arena has 1 560 of them: sixteen waves keep them all in
// flight at once), a shuffle tree per wave, the waves through LDS.  A region without chunks gets (0, 0).
__global__ __launch_bounds__(FIN_BLOCK) void k_finalize(const Part* __restrict__ parts, const int32_t* __restrict__ region_chunk0,
                                                        int32_t n, uint64_t* __restrict__ digests) {
  __shared__ uint64_t sh[FIN_BLOCK / 64][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const int c0 = region_chunk0[r], c1 = region_chunk0[r + 1];
    uint64_t a = 0, b = 0;
#pragma unroll 4
    for (int i = c0 + (int)threadIdx.x; i < c1; i += FIN_BLOCK) {
      const Part p = parts[i];
      a += p.s1;
      b += p.s2;
    }
    wave_sum(a, b);
    if (lane == 0) { sh[wave][0] = a; sh[wave][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int v = 1; v < FIN_BLOCK / 64; ++v) { a += sh[v][0]; b += sh[v][1]; }
      digests[2 * r] = a;
      digests[2 * r + 1] = b;
    }
    __syncthreads();                                             // sh is reused by the next region
  }
}

static_assert(sizeof(Batch) <= 4096, "the by-value table must fit the kernel arguments");

inline int64_t padded(int64_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

// chunks of a table, or -1 where it is malformed / too long
inline int64_t chunk_count(const RiglStateRegion* regions, int32_t n) {
  int64_t total = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (regions[i].bytes < 0 || (regions[i].bytes & 3)) return -1;
    total += ceil_div64(regions[i].bytes >> 2, CHUNK);
    if (total >= (int64_t)1 << 31) return -1;
  }
  return total;
}
inline size_t index_bytes(int32_t n) { return align_up((size_t)(n + 1) * sizeof(int32_t), 256); }

template <bool GATHER>
int run(const char* who, const RiglStateRegion* regions, int32_t n, void* packed, uint64_t* digests, void* workspace,
        size_t workspace_size, int32_t max_blocks, rigl_stream_t stream) {
  if (n < 0) return fail(RIGL_EINVAL, "%s: n = %d < 0", who, n);
  if (max_blocks < 0) return fail(RIGL_EINVAL, "%s: max_blocks = %d < 0", who, max_blocks);
  if (n > 0 && !regions) return fail(RIGL_EINVAL, "%s: NULL table", who);
  if ((uintptr_t)packed & (uintptr_t)(ALIGN - 1)) return fail(RIGL_EINVAL, "%s: packed not %d-byte aligned", who, (int)ALIGN);
  if ((uintptr_t)digests & 7u) return fail(RIGL_EINVAL, "%s: digests not 8-byte aligned", who);
  if (n > 0 && !digests) return fail(RIGL_EINVAL, "%s: NULL digests", who);
  int64_t total_bytes = 0;
  for (int32_t i = 0; i < n; ++i) {
    const RiglStateRegion& r = regions[i];
    if (r.bytes < 0 || (r.bytes & 3)) return fail(RIGL_EINVAL, "%s: region %d: %lld bytes (negative or no multiple of 4)", who, i, (long long)r.bytes);
    if (r.bytes > 0 && !r.ptr) return fail(RIGL_EINVAL, "%s: region %d: NULL with %lld bytes", who, i, (long long)r.bytes);
    if ((uintptr_t)r.ptr & 3u) return fail(RIGL_EINVAL, "%s: region %d: pointer not 4-byte aligned", who, i);
    total_bytes += padded(r.bytes);
  }
  if (total_bytes > 0 && !packed) return fail(RIGL_EINVAL, "%s: NULL packed", who);
  const int64_t chunks = chunk_count(regions, n);
  if (chunks < 0) return fail(RIGL_EUNSUPPORTED, "%s: the table has 2^31 chunks or more", who);
  if (n == 0) return RIGL_OK;
  const size_t need = index_bytes(n) + align_up((size_t)chunks * sizeof(Part), 256);
  if (!workspace || workspace_size < need)
    return fail(RIGL_EWORKSPACE, "%s: workspace of %zu bytes, need %zu", who, workspace ? workspace_size : (size_t)0, need);
  if ((uintptr_t)workspace & 255u) return fail(RIGL_EINVAL, "%s: workspace not 256-byte aligned", who);

  hipStream_t st = as_stream(stream);
  int32_t* region_chunk0 = static_cast<int32_t*>(workspace);
  Part* parts = reinterpret_cast<Part*>(static_cast<uint8_t*>(workspace) + index_bytes(n));
  const int cap = max_blocks > 0 ? max_blocks : DEFAULT_MAX_BLOCKS;
  int32_t chunk_base = 0;
  int64_t packed_word = 0;
  for (int32_t first = 0; first < n; first += BATCH) {
    Batch B;
    B.n = n - first < BATCH ? n - first : BATCH;
    B.first_region = first;
    B.chunk_base = chunk_base;
    int32_t c = 0;
    for (int32_t i = 0; i < BATCH; ++i) {
      B.chunk0[i] = c;
      if (i < B.n) {
        const RiglStateRegion& r = regions[first + i];
        B.r[i] = Reg{static_cast<uint32_t*>(r.ptr), r.bytes >> 2, packed_word};
        c += (int32_t)ceil_div64(r.bytes >> 2, CHUNK);
        packed_word += padded(r.bytes) >> 2;
      } else {
        B.r[i] = Reg{nullptr, 0, 0};
      }
    }
    B.chunk0[BATCH] = c;
    const int grid = c < 1 ? 1 : (c < cap ? c : cap);            // a batch without chunks still leaves its regions' chunk ranges
    hipLaunchKernelGGL((k_move<GATHER>), dim3(grid), dim3(BLOCK), 0, st, B, static_cast<uint32_t*>(packed), parts, region_chunk0);
    RIGL_CHECK_LAUNCH(who);
    chunk_base += c;
  }
  hipLaunchKernelGGL(k_finalize, dim3(n < cap ? n : cap), dim3(FIN_BLOCK), 0, st, parts, region_chunk0, n, digests);
  RIGL_CHECK_LAUNCH(who);
  return RIGL_OK;
}

}  // namespace kstate
}  // namespace rigl

extern "C" {

size_t rigl_state_packed_bytes(const RiglStateRegion* regions, int32_t n) {
  using namespace rigl::kstate;
  if (n < 0 || (n > 0 && !regions)) return 0;
  int64_t total = 0;
  for (int32_t i = 0; i < n; ++i) {
    if (regions[i].bytes < 0 || (regions[i].bytes & 3)) return 0;
    total += padded(regions[i].bytes);
  }
  return (size_t)total;
}

size_t rigl_state_workspace_bytes(const RiglStateRegion* regions, int32_t n) {
  using namespace rigl::kstate;
  if (n <= 0 || !regions) return 0;
  const int64_t chunks = chunk_count(regions, n);
  if (chunks < 0) return 0;
  return index_bytes(n) + rigl::align_up((size_t)chunks * sizeof(Part), 256);
}

int rigl_state_gather(const RiglStateRegion* regions, int32_t n, void* packed, uint64_t* digests, void* workspace,
                      size_t workspace_size, int32_t max_blocks, rigl_stream_t stream) {
  return rigl::kstate::run<true>("rigl_state_gather", regions, n, packed, digests, workspace, workspace_size, max_blocks, stream);
}

int rigl_state_scatter(const RiglStateRegion* regions, int32_t n, const void* packed, uint64_t* digests, void* workspace,
                       size_t workspace_size, int32_t max_blocks, rigl_stream_t stream) {
  return rigl::kstate::run<false>("rigl_state_scatter", regions, n, const_cast<void*>(packed), digests, workspace, workspace_size,
                                  max_blocks, stream);
}

}  // extern "C"
