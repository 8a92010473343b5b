// gcre_patients.hip -- carrier tallies per patient (gcre_set_patient_counts).
//   * k_set_patient_counts  counts[group][plane][patient] += bit `patient` of the carrier row of every listed set: a column
//                           sum of a bit matrix, in the bit-sliced counters of gcre_bitslice.h
// The context-side entry (the counting sort by group, the member table, the segments) is in gcre_host_stats.hip.
//
// One wave owns one (segment, tile of 64 dwords = 2,048 patients); a lane owns one dword column.  For 16 entries at a time
// the lane ORs each entry's member dwords -- k_clump_union's mapping (gcre_clump.hip): the member indices are wave-uniform
// scalar loads (the table is stored member column by member column, so the 16 entries of a batch are 64 contiguous
// bytes), every member's dword is one coalesced vector load, the last dword is masked to the patients -- and feeds the 16
// words to add16<kPatientPlanes>; a tail of fewer than 16 goes through add4 in fours, padded with zero words.  The
// planes are flushed before they can overflow and at the end of the segment: the 32 counts of a lane go through a
// per-wave LDS stage so that every atomic wave-instruction covers 64 consecutive cells, and are added with no-return
// 32-bit integer atomics -- the sums do not depend on the order.  Blocks are numbered with the segment running fastest
// and the tile slowest, so that the waves resident at one time read the same 256-byte slice of the gene rows.
#include "gcre_kernels.h"
#include "gcre_bitslice.h"

namespace gcre {
namespace {

constexpr int kPcBlock = 256;              // four waves, one (segment, tile) each
constexpr int kPcWaves = kPcBlock / 64;
constexpr int kPcStride = 33;              // dwords per lane of the flush stage: odd, so a lane's 32 counts fan out over the banks
constexpr int kPcCap = (1 << kPatientPlanes) - 1;   // entries the planes hold

static_assert(kPatientTile == 64 * 32 && kPatientPlanes >= 5 && kPatientPlanes <= 30, "tile and plane shape");

// The planes' 32 counts per lane, added to cells[0 .. 2047] of this tile (`left` of them exist), then the planes cleared.
__device__ __forceinline__ void pc_flush(u32 (&P)[kPatientPlanes], u32* stage, u32* cells, int left, int lane) {
#pragma unroll
  for (int b = 0; b < 32; b++) {
    u32 c = 0;
#pragma unroll
    for (int l = 0; l < kPatientPlanes; l++) c |= ((P[l] >> b) & 1u) << l;
    stage[lane * kPcStride + b] = c;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 4
  for (int k = 0; k < 32; k++) {
    const int idx = k * 64 + lane;   // the patient within the tile: lane idx / 32, bit idx % 32
    const u32 v = stage[(idx >> 5) * kPcStride + (idx & 31)];
    if (idx < left && v != 0u) atomicAdd(cells + idx, v);
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();   // the stage is written again by the next flush
#pragma unroll
  for (int l = 0; l < kPatientPlanes; l++) P[l] = 0u;
}

}  // namespace

// grid: one wave per (segment, tile), 4 per block; wave id = tile * nseg + segment
template <int H>
__global__ __launch_bounds__(kPcBlock) void k_set_patient_counts(const PatientCountArgs a) {
  __shared__ u32 s_stage[kPcWaves][64 * kPcStride];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  const i64 ntiles = (a.n_patients + kPatientTile - 1) / kPatientTile;
  const i64 id = (i64)blockIdx.x * kPcWaves + wave;
  if (id >= a.nseg * ntiles) return;   // the whole wave
  const int tile = (int)(id / a.nseg);
  const PatientSeg GCRE_CONSTANT* segp = (const PatientSeg GCRE_CONSTANT*)a.segs + id % a.nseg;
  PatientSeg sg;
  sg.begin = segp->begin;
  sg.count = segp->count;
  sg.group = segp->group;
  sg.width = segp->width;
  const int w = tile * 64 + lane;
  const bool live = w < a.W2 && w * 32 < a.n_patients;
  const int wl = live ? w : 0;                           // a lane without patients reads column 0 and keeps nothing
  const int lane_left = a.n_patients - w * 32;           // patients from this dword on
  const u32 mask = !live ? 0u : lane_left < 32 ? (1u << lane_left) - 1u : 0xffffffffu;
  const int left = a.n_patients - tile * kPatientTile;   // patients from this tile on (> 0)
  u32* stage = s_stage[wave];
  u32* cells = a.cells + (i64)sg.group * H * a.n_patients + (i64)tile * kPatientTile;

  u32 P[kPatientPlanes], N[kPatientPlanes];
#pragma unroll
  for (int l = 0; l < kPatientPlanes; l++) P[l] = N[l] = 0u;

  // entry e's words: every member's dword ORed into xp (by_sign: into xn where the entry's sign bit is set); a -1 behind
  // the last member reads row 0 and keeps nothing, so that the 16 loads of a member column are issued together
  const int32_t GCRE_CONSTANT* members = (const int32_t GCRE_CONSTANT*)a.members;
  auto gather = [&](const i64 e, const int m, u32& xp, u32& xn) {
    const int32_t g = members[(i64)m * a.n + e];
    const int32_t row = g < 0 ? 0 : (g & ~kPatientNegBit);
    const bool neg = H == 2 && g >= 0 && (g & kPatientNegBit);
    const u32 v = a.rows[(i64)row * a.W2 + wl];
    xp |= (g < 0 || neg) ? 0u : v;
    if (H == 2) xn |= neg ? v : 0u;
  };

  i64 e = sg.begin;
  const i64 end = e + sg.count;
  int pending = 0;   // entries in the planes
  auto flush = [&]() {
    pc_flush(P, stage, cells, left, lane);
    if (H == 2) pc_flush(N, stage, cells + a.n_patients, left, lane);
    pending = 0;
  };
  for (; e + 16 <= end; e += 16) {
    if (pending + 16 > kPcCap) flush();
    u32 xp[16], xn[16];
#pragma unroll
    for (int j = 0; j < 16; j++) xp[j] = xn[j] = 0u;
    for (int m = 0; m < sg.width; m++) {
#pragma unroll
      for (int j = 0; j < 16; j++) gather(e + j, m, xp[j], xn[j]);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) {
      xp[j] &= mask;
      xn[j] &= mask;
    }
    add16<kPatientPlanes>(P, xp);
    if (H == 2) add16<kPatientPlanes>(N, xn);
    pending += 16;
  }
  for (; e < end; e += 4) {   // the tail in fours; the words past the end stay zero
    if (pending + 4 > kPcCap) flush();
    u32 xp[4] = {0u, 0u, 0u, 0u}, xn[4] = {0u, 0u, 0u, 0u};
    for (int m = 0; m < sg.width; m++) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (e + j < end) gather(e + j, m, xp[j], xn[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      xp[j] &= mask;
      xn[j] &= mask;
    }
    add4<kPatientPlanes>(P, xp);
    if (H == 2) add4<kPatientPlanes>(N, xn);
    pending += 4;
  }
  if (pending > 0) flush();
}

// one wave per (segment, tile); a grid that does not fit is refused, never clamped
hipError_t launch_set_patient_counts(const PatientCountArgs& a, hipStream_t stream) {
  if (a.nseg == 0 || a.n_patients == 0) return hipSuccess;
  if (a.nseg < 0 || a.n_patients < 0 || a.n < a.nseg || a.M < 1 || a.W2 < 1 || (i64)a.W2 * 32 < a.n_patients || (a.H != 1 && a.H != 2))
    return hipErrorInvalidValue;
  const i64 ntiles = (a.n_patients + kPatientTile - 1) / kPatientTile;
  if (a.nseg > ((i64)0x7fffffff * kPcWaves) / ntiles) return hipErrorInvalidValue;
  const i64 blocks = (a.nseg * ntiles + kPcWaves - 1) / kPcWaves;
  if (g_launch_trace)
    fprintf(stderr, "launch k_set_patient_counts segments=%lld tiles=%lld blocks=%lld\n", (long long)a.nseg, (long long)ntiles, (long long)blocks);
  if (a.H == 1) hipLaunchKernelGGL(k_set_patient_counts<1>, dim3((unsigned)blocks), dim3(kPcBlock), 0, stream, a);
  else hipLaunchKernelGGL(k_set_patient_counts<2>, dim3((unsigned)blocks), dim3(kPcBlock), 0, stream, a);
  return hipGetLastError();
}

}  // namespace gcre
