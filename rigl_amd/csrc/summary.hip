// Per-step training summaries: one read-only pass over the weight and gradient arenas that leaves, per trainable variable,
// the sums and counts the reference's drivers log every step (imagenet_train_eval.py:431-473, utils.py:59-90) in a device ring.
//   rigl_summary_step : partials per fixed-size chunk (one launch per RIGL_SUMMARY_BATCH entries, the table by value), then ONE
//                       finalize launch: chunk partials -> entries -> totals -> the record of slot *step % ring_slots; *step += 1
// The reduction tree is a function of the table alone: a chunk is RIGL_SUMMARY_CHUNK elements of one entry, reduced by one
// workgroup in a fixed order (lane-sequential, a fixed shuffle tree, the four waves in order); the finalize sums an entry's
// chunks in chunk order (one lane for a short entry; lane-strided through the same tree for a long one: the entry's chunk
// count decides), and the entries lane-strided through the tree.  The grid only decides which workgroup
// takes which chunk.  No atomics, no cross-workgroup hand-off inside a launch, plain vector loads and stores.
#include "common.hpp"

// The gradient is K3's (optimizer.hip masked_grad): every fp32 product / sum rounded separately.
#pragma clang fp contract(off)

namespace rigl {
namespace ksum {

constexpr int BLOCK = 256;
constexpr int CHUNK = RIGL_SUMMARY_CHUNK;
constexpr int BATCH = 64;            // entries per partials launch: the by-value table stays under the 4 KiB of kernel arguments
constexpr int FIN_BLOCK = 1024;      // the finalize workgroup: 16 waves
constexpr int FIN_SMALL = 8;         // entries of up to this many chunks are summed by one lane, longer ones by a wave
constexpr int HEADER_BYTES = 16;     // int32 step, int32 n_entries, fp32 loss, fp32 learning rate
constexpr int GROUP_BYTES = 48;      // fp64 sumsq_g, sumsq_w, l1_w; int64 nz_w, mask_ones, nonfinite_g

static_assert(CHUNK % (4 * BLOCK) == 0 && CHUNK % 32 == 0, "a chunk is whole quads per lane and whole mask words");
static_assert(CHUNK <= (1 << 20), "three chunk counts share one 64-bit word, 21 bits each");

struct Ent {
  const float* w;
  const float* g;
  const uint32_t* mask;
  int64_t n;
  float wd;
  int32_t apply_mask;
};

struct Batch {
  Ent e[BATCH];
  int32_t chunk0[BATCH + 1];  // first chunk of entry i inside this batch; [n] = the batch's chunk count
  int32_t n;                  // entries in this batch
  int32_t first_entry;        // index of e[0] in the caller's table
  int32_t chunk_base;         // chunks of the batches in front
  float gscale;
};

struct Part {                 // one chunk
  double s[3];                // sumsq_g, sumsq_w, l1_w
  uint64_t counts;            // nz_w | mask_ones << 21 | nonfinite_g << 42
};

struct Acc {
  double sg, sw, l1;
  uint32_t nz, ones, nf;
};

// gq = f32(f32(m * f32(gscale * g)) + f32(wd * w)) with K3's rule for a masked-off element (the signed zero of the scaled
// gradient, taken from the bits: a non-finite gradient there counts as that zero too).  `on` is the mask bit where the entry
// applies its mask, else true; `bit` is the mask bit itself (what mask_ones counts).
__device__ __forceinline__ void acc_one(Acc& a, float w, float g, bool on, bool bit, float gscale, float wd) {
  const float gs = __fmul_rn(g, gscale);
  const float gm = on ? gs : __uint_as_float(__float_as_uint(gs) & 0x80000000u);
  const float gq = __fadd_rn(gm, __fmul_rn(wd, w));
  const double dg = (double)gq, dw = (double)w;   // squares and magnitudes of fp32 values are exact in fp64
  a.sg += dg * dg;
  a.sw += dw * dw;
  a.l1 += fabs(dw);
  a.nz += (__float_as_uint(w) & 0x7FFFFFFFu) != 0u;             // -0.0 is zero, subnormals are not
  a.ones += bit;
  a.nf += (__float_as_uint(gq) & 0x7F800000u) == 0x7F800000u;   // inf or NaN
}

__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int off) {
  const uint32_t lo = __shfl_down((uint32_t)v, off, 64), hi = __shfl_down((uint32_t)(v >> 32), off, 64);
  return ((uint64_t)hi << 32) | lo;
}

// The fixed wave tree: lane l += lane l + off for off = 32, 16 .. 1; lane 0 ends with the wave's sum.
__device__ __forceinline__ void wave_tree(double& a, double& b, double& c) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b += __shfl_down(b, off, 64);
    c += __shfl_down(c, off, 64);
  }
}
__device__ __forceinline__ void wave_tree(uint64_t& v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += shfl_down_u64(v, off);
}

__global__ __launch_bounds__(BLOCK) void k_partials(Batch B, Part* __restrict__ parts, int32_t* __restrict__ entry_chunk0) {
  __shared__ double sh[BLOCK / 64][3];
  __shared__ uint64_t shc[BLOCK / 64];
  // the chunk range of every entry of this batch, for the finalize launch (index first_entry + n is written again, with the
  // same value, by the next batch)
  if (blockIdx.x == 0 && (int)threadIdx.x <= B.n) entry_chunk0[B.first_entry + threadIdx.x] = B.chunk_base + B.chunk0[threadIdx.x];
  const int total = B.chunk0[B.n];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = blockIdx.x; c < total; c += gridDim.x) {
    int lo = 0, hi = B.n - 1;                    // the last entry whose first chunk is <= c (empty entries share a start: skipped)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (B.chunk0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    const Ent E = B.e[lo];
    const int64_t base = (int64_t)(c - B.chunk0[lo]) * CHUNK;
    const int64_t left = E.n - base;
    const int m = left < CHUNK ? (int)left : CHUNK;              // elements of this chunk: [base, base + m) inside [0, n)
    const float* __restrict__ w = E.w + base;
    const float* __restrict__ g = E.g + base;
    const uint32_t* __restrict__ mask = E.mask ? E.mask + (base >> 5) : nullptr;
    const bool apply = E.apply_mask != 0;
    Acc a = {0.0, 0.0, 0.0, 0u, 0u, 0u};
    const int nq = m >> 2;                                       // whole quads; the padding behind n is never read
#pragma unroll 4
    for (int q = threadIdx.x; q < nq; q += BLOCK) {
      const int e = q << 2;
      const float4 wv = *reinterpret_cast<const float4*>(w + e);
      const float4 gv = *reinterpret_cast<const float4*>(g + e);
      const uint32_t nib = mask ? (mask[e >> 5] >> (uint32_t)(e & 31)) & 0xFu : 0xFu;
      acc_one(a, wv.x, gv.x, !apply || (nib & 1u), nib & 1u, B.gscale, E.wd);
      acc_one(a, wv.y, gv.y, !apply || (nib & 2u), nib & 2u, B.gscale, E.wd);
      acc_one(a, wv.z, gv.z, !apply || (nib & 4u), nib & 4u, B.gscale, E.wd);
      acc_one(a, wv.w, gv.w, !apply || (nib & 8u), nib & 8u, B.gscale, E.wd);
    }
    if ((int)threadIdx.x < (m & 3)) {                            // the last n % 4 elements, one lane each, after that lane's quads
      const int e = (nq << 2) + threadIdx.x;
      const bool bit = mask ? ((mask[e >> 5] >> (uint32_t)(e & 31)) & 1u) != 0u : true;
      acc_one(a, w[e], g[e], !apply || bit, bit, B.gscale, E.wd);
    }
    uint64_t cnt = (uint64_t)a.nz | ((uint64_t)a.ones << 21) | ((uint64_t)a.nf << 42);
    wave_tree(a.sg, a.sw, a.l1);
    wave_tree(cnt);
    if (lane == 0) {
      sh[wave][0] = a.sg; sh[wave][1] = a.sw; sh[wave][2] = a.l1;
      shc[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      Part p;
      p.s[0] = sh[0][0]; p.s[1] = sh[0][1]; p.s[2] = sh[0][2];
      p.counts = shc[0];
#pragma unroll
      for (int v = 1; v < BLOCK / 64; ++v) {                     // the waves in order
        p.s[0] += sh[v][0]; p.s[1] += sh[v][1]; p.s[2] += sh[v][2];
        p.counts += shc[v];
      }
      parts[B.chunk_base + c] = p;
    }
    __syncthreads();                                             // sh is reused by the next chunk
  }
}

struct Group {                // an entry's outputs, and the totals: GROUP_BYTES in the record
  double s[3];
  int64_t c[3];
};

struct FinArgs {
  const Part* parts;
  const int32_t* entry_chunk0;
  int32_t n_entries;
  int32_t ring_slots;
  uint8_t* ring;
  size_t slot_bytes;
  int32_t* step;
  const float* loss;          // nullable
  const float* lr_dev;        // nullable: then lr
  float lr;
};

__global__ __launch_bounds__(FIN_BLOCK) void k_finalize(FinArgs A) {
  const int32_t s = *A.step;                                     // every lane reads it in front of the barrier; lane 0 writes behind it
  const int32_t slot = ((s % A.ring_slots) + A.ring_slots) % A.ring_slots;
  uint8_t* rec = A.ring + (size_t)slot * A.slot_bytes;
  Group* totals = reinterpret_cast<Group*>(rec + HEADER_BYTES);
  Group* ent = totals + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int WAVES = FIN_BLOCK / 64;
  // Entries of at most FIN_SMALL chunks (every batch-norm vector, most kernels of a CIFAR model): one LANE per entry, its
  // chunks summed in chunk order -- all of a lane's loads are in flight together.
  for (int e = threadIdx.x; e < A.n_entries; e += FIN_BLOCK) {
    const int c0 = A.entry_chunk0[e], nc = A.entry_chunk0[e + 1] - c0;
    if (nc > FIN_SMALL) continue;
    Part p[FIN_SMALL];
#pragma unroll
    for (int k = 0; k < FIN_SMALL; ++k)
      if (k < nc) p[k] = A.parts[c0 + k];
    Group o = {{0.0, 0.0, 0.0}, {0, 0, 0}};
#pragma unroll
    for (int k = 0; k < FIN_SMALL; ++k)
      if (k < nc) {
        o.s[0] += p[k].s[0]; o.s[1] += p[k].s[1]; o.s[2] += p[k].s[2];
        o.c[0] += (int64_t)(p[k].counts & 0x1FFFFFu); o.c[1] += (int64_t)((p[k].counts >> 21) & 0x1FFFFFu);
        o.c[2] += (int64_t)(p[k].counts >> 42);
      }
    ent[e] = o;
  }
  // The longer entries: one WAVE per entry at a time (entries wave, wave + WAVES ...), its chunks lane-strided, in chunk
  // order, then the wave tree.  The chunk ranges of the wave's next 64 entries are fetched by its 64 lanes in one round trip
  // and handed out by shuffles.
  for (int e0 = wave; e0 < A.n_entries; e0 += 64 * WAVES) {
    const int mine = e0 + WAVES * lane;
    int my0 = 0, my1 = 0;
    if (mine < A.n_entries) { my0 = A.entry_chunk0[mine]; my1 = A.entry_chunk0[mine + 1]; }
    for (int j = 0; j < 64; ++j) {
      const int e = e0 + WAVES * j;
      if (e >= A.n_entries) break;
      const int c0 = __shfl(my0, j, 64), c1 = __shfl(my1, j, 64);
      if (c1 - c0 <= FIN_SMALL) continue;
      double a = 0.0, b = 0.0, c = 0.0;
      uint64_t nz = 0, ones = 0, nf = 0;
      for (int i = c0 + lane; i < c1; i += 64) {
        const Part p = A.parts[i];
        a += p.s[0]; b += p.s[1]; c += p.s[2];
        nz += p.counts & 0x1FFFFFu; ones += (p.counts >> 21) & 0x1FFFFFu; nf += p.counts >> 42;
      }
      wave_tree(a, b, c);
      wave_tree(nz); wave_tree(ones); wave_tree(nf);
      if (lane == 0) {
        Group o;
        o.s[0] = a; o.s[1] = b; o.s[2] = c;
        o.c[0] = (int64_t)nz; o.c[1] = (int64_t)ones; o.c[2] = (int64_t)nf;
        ent[e] = o;
      }
    }
  }
  __syncthreads();                                            // the entries of this record, written by this workgroup, are read back
  if (wave != 0) return;
  double a = 0.0, b = 0.0, c = 0.0;
  uint64_t nz = 0, ones = 0, nf = 0;
  for (int e = lane; e < A.n_entries; e += 64) {                 // the totals: the entries lane-strided, in entry order
    const Group o = ent[e];
    a += o.s[0]; b += o.s[1]; c += o.s[2];
    nz += (uint64_t)o.c[0]; ones += (uint64_t)o.c[1]; nf += (uint64_t)o.c[2];
  }
  wave_tree(a, b, c);
  wave_tree(nz); wave_tree(ones); wave_tree(nf);
  if (lane == 0) {
    Group t;
    t.s[0] = a; t.s[1] = b; t.s[2] = c;
    t.c[0] = (int64_t)nz; t.c[1] = (int64_t)ones; t.c[2] = (int64_t)nf;
    *totals = t;
    int32_t* hi = reinterpret_cast<int32_t*>(rec);
    float* hf = reinterpret_cast<float*>(rec);
    hi[0] = s;
    hi[1] = A.n_entries;
    hf[2] = A.loss ? *A.loss : __uint_as_float(0x7FC00000u);     // no loss given: NaN
    hf[3] = A.lr_dev ? *A.lr_dev : A.lr;
    *A.step = (int32_t)((uint32_t)s + 1u);                       // int32 wrap-around, as k_lr_schedule_step
  }
}

static_assert(sizeof(Group) == GROUP_BYTES, "record layout");
static_assert(sizeof(Batch) <= 4096, "the by-value table must fit the kernel arguments");

// chunks of a table, or -1 where it is malformed / too long
inline int64_t chunk_count(const RiglSummaryEntry* entries, int32_t n_entries) {
  int64_t total = 0;
  for (int32_t i = 0; i < n_entries; ++i) {
    if (entries[i].n < 0) return -1;
    total += ceil_div64(entries[i].n, CHUNK);
    if (total >= (int64_t)1 << 31) return -1;
  }
  return total;
}
inline size_t index_bytes(int32_t n_entries) { return align_up((size_t)(n_entries + 1) * sizeof(int32_t), 256); }

}  // namespace ksum
}  // namespace rigl

extern "C" {

size_t rigl_summary_slot_bytes(int32_t n_entries) {
  using namespace rigl::ksum;
  if (n_entries < 0) return 0;
  return rigl::align_up((size_t)HEADER_BYTES + (size_t)GROUP_BYTES * ((size_t)n_entries + 1), 64);
}

size_t rigl_summary_workspace_bytes(const RiglSummaryEntry* entries, int32_t n_entries) {
  using namespace rigl::ksum;
  if (n_entries < 0 || (n_entries > 0 && !entries)) return 0;
  const int64_t chunks = chunk_count(entries, n_entries);
  if (chunks < 0) return 0;
  return index_bytes(n_entries) + rigl::align_up((size_t)chunks * sizeof(Part), 256);
}

int rigl_summary_step(const RiglSummaryEntry* entries, int32_t n_entries, float grad_scale, const float* loss,
                      const float* lr, float lr_value, int32_t* step, void* ring, int32_t ring_slots, void* workspace,
                      size_t workspace_size, int32_t max_blocks, rigl_stream_t stream) {
  using namespace rigl;
  using namespace rigl::ksum;
  if (n_entries < 0 || (n_entries > 0 && !entries)) return fail(RIGL_EINVAL, "rigl_summary_step: NULL table / negative n_entries");
  if (!step || !ring) return fail(RIGL_EINVAL, "rigl_summary_step: NULL step / ring");
  if (ring_slots < 1) return fail(RIGL_EINVAL, "rigl_summary_step: ring_slots %d < 1", ring_slots);
  if (max_blocks < 0) return fail(RIGL_EINVAL, "rigl_summary_step: negative max_blocks");
  if (((uintptr_t)step | (uintptr_t)loss | (uintptr_t)lr) & 3u)
    return fail(RIGL_EINVAL, "rigl_summary_step: step / loss / lr not 4-byte aligned");
  if ((uintptr_t)ring & 15u) return fail(RIGL_EINVAL, "rigl_summary_step: ring not 16-byte aligned");
  for (int32_t i = 0; i < n_entries; ++i) {
    const RiglSummaryEntry& e = entries[i];
    if (e.n < 0) return fail(RIGL_EINVAL, "rigl_summary_step: entry %d: negative n", i);
    if (e.n > 0 && (!e.w || !e.g)) return fail(RIGL_EINVAL, "rigl_summary_step: entry %d: NULL w / g", i);
    if (((uintptr_t)e.w | (uintptr_t)e.g) & 15u) return fail(RIGL_EINVAL, "rigl_summary_step: entry %d: w / g not 16-byte aligned", i);
    if ((uintptr_t)e.mask_bits & 3u) return fail(RIGL_EINVAL, "rigl_summary_step: entry %d: mask_bits not 4-byte aligned", i);
  }
  const int64_t chunks = chunk_count(entries, n_entries);
  if (chunks < 0) return fail(RIGL_EUNSUPPORTED, "rigl_summary_step: the table has 2^31 chunks or more");
  const size_t need = rigl_summary_workspace_bytes(entries, n_entries);
  if (!workspace || workspace_size < need)
    return fail(RIGL_EWORKSPACE, "rigl_summary_step: workspace of %zu bytes, need %zu", workspace ? workspace_size : (size_t)0, need);
  if ((uintptr_t)workspace & 255u) return fail(RIGL_EINVAL, "rigl_summary_step: workspace not 256-byte aligned");

  hipStream_t st = as_stream(stream);
  int32_t* entry_chunk0 = static_cast<int32_t*>(workspace);
  Part* parts = reinterpret_cast<Part*>(static_cast<uint8_t*>(workspace) + index_bytes(n_entries));
  const int cap = max_blocks > 0 ? max_blocks : INT32_MAX;       // default: a workgroup per chunk, balanced by the dispatcher
  int32_t chunk_base = 0;
  for (int32_t first = 0; first < n_entries; first += BATCH) {
    Batch B;
    B.n = n_entries - first < BATCH ? n_entries - first : BATCH;
    B.first_entry = first;
    B.chunk_base = chunk_base;
    B.gscale = grad_scale;
    int32_t c = 0;
    for (int32_t i = 0; i < BATCH; ++i) {
      B.chunk0[i] = c;
      if (i < B.n) {
        const RiglSummaryEntry& e = entries[first + i];
        B.e[i] = Ent{e.w, e.g, e.mask_bits, e.n, e.weight_decay, e.apply_mask};
        c += (int32_t)ceil_div64(e.n, CHUNK);
      } else {
        B.e[i] = Ent{nullptr, nullptr, nullptr, 0, 0.f, 0};
      }
    }
    B.chunk0[BATCH] = c;
    const int grid = c < 1 ? 1 : (c < cap ? c : cap);            // an empty batch still leaves its entries' chunk ranges
    hipLaunchKernelGGL(k_partials, dim3(grid), dim3(BLOCK), 0, st, B, parts, entry_chunk0);
    RIGL_CHECK_LAUNCH("rigl_summary_step (partials)");
    chunk_base += c;
  }
  FinArgs A;
  A.parts = parts;
  A.entry_chunk0 = entry_chunk0;
  A.n_entries = n_entries;
  A.ring_slots = ring_slots;
  A.ring = static_cast<uint8_t*>(ring);
  A.slot_bytes = rigl_summary_slot_bytes(n_entries);
  A.step = step;
  A.loss = loss;
  A.lr_dev = lr;
  A.lr = lr_value;
  hipLaunchKernelGGL(k_finalize, dim3(1), dim3(FIN_BLOCK), 0, st, A);
  RIGL_CHECK_LAUNCH("rigl_summary_step (finalize)");
  return RIGL_OK;
}

}  // extern "C"
