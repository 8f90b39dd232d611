// Multi-scale test augmentation: the merge of CenterNet's test code, `soft_nms(..., Nt=0.5, method=2)` per class over the
// union of the passes' detections, then the per-image cap.  The rule is written out in DESIGN.md 7.10; what matters here:
//
//   * the passes are read IN PLACE: the kernel arguments carry a table of per-pass pointers and widths (ctdet_softnms_pass,
//     at most SN_MAX_PASSES), the counts are read on the device.  A candidate's index is its position in the pass-major
//     concatenation, `offset of its pass + k`; only the order of the indices matters.
//   * sn_cell_kernel: ONE WAVE per (image, class) cell.  The wave scans the image's candidates, compacts those of its class
//     into LDS in index order (ballot + prefix popcount), then runs the greedy loop: every lane keeps the live flags of its
//     slots (slot = lane + 64 t) as one bit mask in a register, the pick is a wave maximum over the 64-bit key
//     {monotone(score), ~slot} -- highest score, ties to the lowest index, a total order whatever the scores hold -- and every
//     lane decays its own live slots against the picked box, which all lanes read from the same LDS address.
//     It writes, at the candidate's own index of the workspace, the score the candidate was selected with and its selection
//     order within the class, or order -1 when the decay removed it.  No two cells write the same index: no atomics.
//   * sn_rank_kernel: one workgroup per image.  Every survivor gets the 64-bit key {~monotone(score), class, selection order}
//     (all distinct), its rank is the number of smaller keys (LDS, every thread reads the same key at a time), and the
//     survivors of rank < max_det are written at their rank.  The tail of the outputs is zeroed, the count is the number
//     written, or -1 when any pass flagged the image as non-finite (count -1).
//   * f32 arithmetic in the order of the definition; compiled with floating point contraction OFF (FLAGS_softnms): the error
//     bound of tests/soft_nms_cases.py counts one rounding per operation.  exp is the library's expf (<= 1 ulp).
//   * the only atomic is an integer add in LDS (the survivor count): two runs are bit-identical.
#include "common.h"
#include "../../include/ctdet_hip.h"

#define SN_MAX_PASSES CTDET_SOFTNMS_MAX_PASSES
#define SN_MAX_CAND CTDET_SOFTNMS_MAX_CANDIDATES
#define SN_SLOTS (SN_MAX_CAND / 64)   // live bits a lane holds
#define SN_NT 256                     // rank workgroup
static_assert(SN_SLOTS <= 32, "a lane's live flags are one 32-bit mask");

struct SnArgs {
  ctdet_softnms_pass pass[SN_MAX_PASSES];
  int npass, B, C, N, max_det;      // N: the sum of the passes' widths (candidate indices are < N)
  float sigma, min_score;
  float* ws_score; int* ws_order;   // [B, N]
  float* out_boxes; float* out_scores; int* out_classes; int* out_counts;
};

// ascending key = ascending score; -0 == +0
__device__ __forceinline__ uint32_t sn_score_key(float s) {
  const uint32_t u = __float_as_uint(s + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long sn_wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

__global__ void __launch_bounds__(64) sn_cell_kernel(SnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sn_lds[];
  float4* box = (float4*)sn_lds;          // [N] the cell's candidates, in index order
  float* sc = (float*)(box + a.N);        // [N] current scores
  int* id = (int*)(sc + a.N);             // [N] candidate indices
  const int b = blockIdx.x / a.C, c = blockIdx.x % a.C, lane = threadIdx.x;
  int n = 0, off = 0;
  for (int s = 0; s < a.npass; ++s) {
    const ctdet_softnms_pass p = a.pass[s];
    int cnt = p.counts[b];
    if (cnt < 0) return;                  // a non-finite pass: sn_rank_kernel flags the image (uniform: the whole wave leaves)
    cnt = cnt < p.K ? cnt : p.K;
    const long row = (long)b * p.K;
    for (int k0 = 0; k0 < cnt; k0 += 64) {
      const int k = k0 + lane;
      const bool mine = k < cnt && p.classes[row + k] == c;
      const unsigned long long m = __ballot(mine);
      if (mine) {
        const int pos = n + __popcll(m & ((1ull << lane) - 1ull));
        const float* bp = p.boxes + (row + k) * 4;
        box[pos] = make_float4(bp[0], bp[1], bp[2], bp[3]);
        sc[pos] = p.scores[row + k];
        id[pos] = off + k;
      }
      n += __popcll(m);
    }
    off += p.K;
  }
  if (n == 0) return;
  __syncthreads();
  float* wsc = a.ws_score + (long)b * a.N;
  int* wor = a.ws_order + (long)b * a.N;
  const int mine_n = n > lane ? (n - lane + 63) / 64 : 0;               // slots lane, lane + 64, ... below n
  uint32_t live = mine_n >= 32 ? 0xFFFFFFFFu : ((1u << mine_n) - 1u);
  for (int sel = 0;; ++sel) {
    unsigned long long best = 0;                                        // 0: no live slot (a key's low word is >= ~SN_MAX_CAND)
    for (uint32_t w = live; w; w &= w - 1) {
      const int j = lane + 64 * (__ffs(w) - 1);
      const unsigned long long key = ((unsigned long long)sn_score_key(sc[j]) << 32) | (0xFFFFFFFFu - (uint32_t)j);
      best = key > best ? key : best;
    }
    best = sn_wave_max(best);
    if (best == 0) break;
    const int m = (int)(0xFFFFFFFFu - (uint32_t)best);
    const float4 bm = box[m];
    const float sm = sc[m];
    if ((m & 63) == lane) {
      live &= ~(1u << (m >> 6));
      const int cm = id[m];
      wsc[cm] = sm;
      wor[cm] = sel;
    }
    const float am = (bm.z - bm.x + 1.f) * (bm.w - bm.y + 1.f);
    for (uint32_t w = live; w; w &= w - 1) {
      const int t = __ffs(w) - 1, j = lane + 64 * t;
      const float4 bi = box[j];
      const float iw = fminf(bm.z, bi.z) - fmaxf(bm.x, bi.x) + 1.f;
      const float ih = fminf(bm.w, bi.w) - fmaxf(bm.y, bi.y) + 1.f;
      if (iw > 0.f && ih > 0.f) {
        const float inter = iw * ih;
        const float ua = am + (bi.z - bi.x + 1.f) * (bi.w - bi.y + 1.f) - inter;
        const float ov = inter / ua;
        const float s = sc[j] * expf(-(ov * ov) / a.sigma);
        sc[j] = s;
        if (s < a.min_score) {
          live &= ~(1u << t);
          wor[id[j]] = -1;
        }
      }
    }
    __syncthreads();      // the decayed scores are in LDS before the next pick reads sc[m] of another lane's slot
  }
}

__global__ void __launch_bounds__(SN_NT) sn_rank_kernel(SnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sn_lds[];
  unsigned long long* keys = (unsigned long long*)sn_lds;      // [N]; ~0: not a survivor
  __shared__ int s_count;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_count = 0;
  __syncthreads();
  bool bad = false;
  for (int s = 0; s < a.npass; ++s) bad |= a.pass[s].counts[b] < 0;
  const float* wsc = a.ws_score + (long)b * a.N;
  const int* wor = a.ws_order + (long)b * a.N;
  int off = 0, local = 0;
  for (int s = 0; s < a.npass; ++s) {
    const ctdet_softnms_pass p = a.pass[s];
    int cnt = bad ? 0 : p.counts[b];
    cnt = cnt < p.K ? cnt : p.K;
    for (int k = tid; k < p.K; k += SN_NT) {
      unsigned long long key = ~0ull;
      if (k < cnt) {
        const int c = p.classes[(long)b * p.K + k];
        if (c >= 0 && c < a.C) {
          const int o = wor[off + k];
          if (o >= 0) {
            key = ((unsigned long long)(~sn_score_key(wsc[off + k])) << 32) | ((unsigned long long)(uint32_t)c << 11) | (uint32_t)o;
            ++local;
          }
        }
      }
      keys[off + k] = key;
    }
    off += p.K;
  }
  if (local) atomicAdd(&s_count, local);
  __syncthreads();
  const int kept = s_count < a.max_det ? s_count : a.max_det;
  float* ob = a.out_boxes + (long)b * a.max_det * 4;
  float* os = a.out_scores + (long)b * a.max_det;
  int* oc = a.out_classes + (long)b * a.max_det;
  for (int r = kept + tid; r < a.max_det; r += SN_NT) {
    ob[r * 4L] = 0.f; ob[r * 4L + 1] = 0.f; ob[r * 4L + 2] = 0.f; ob[r * 4L + 3] = 0.f;
    os[r] = 0.f;
    oc[r] = 0;
  }
  if (tid == 0) a.out_counts[b] = bad ? -1 : kept;
  off = 0;
  for (int s = 0; s < a.npass; ++s) {
    const ctdet_softnms_pass p = a.pass[s];
    for (int k = tid; k < p.K; k += SN_NT) {
      const unsigned long long key = keys[off + k];
      if (key == ~0ull) continue;
      int rank = 0;
      for (int i = 0; i < a.N; ++i) rank += keys[i] < key;
      if (rank < a.max_det) {
        const float* bp = p.boxes + ((long)b * p.K + k) * 4;
        ob[rank * 4L] = bp[0]; ob[rank * 4L + 1] = bp[1]; ob[rank * 4L + 2] = bp[2]; ob[rank * 4L + 3] = bp[3];
        os[rank] = wsc[off + k];
        oc[rank] = p.classes[(long)b * p.K + k];
      }
    }
    off += p.K;
  }
}

int launch_soft_nms(const ctdet_softnms_pass* passes, int npass, int B, int C, float sigma, float min_score, int max_det,
                    void* workspace, float* out_boxes, float* out_scores, int* out_classes, int* out_counts, hipStream_t s) {
  SnArgs a = {};
  int N = 0;
  for (int i = 0; i < npass; ++i) { a.pass[i] = passes[i]; N += passes[i].K; }
  CTDET_KERNEL("sn_cell_kernel<wave per (image,class)> + sn_rank_kernel<workgroup per image>: %d passes, %d candidates", npass, N);
  if (B == 0) return 0;
  a.npass = npass; a.B = B; a.C = C; a.N = N; a.max_det = max_det; a.sigma = sigma; a.min_score = min_score;
  a.ws_score = (float*)workspace; a.ws_order = (int*)workspace + (long)B * N;
  a.out_boxes = out_boxes; a.out_scores = out_scores; a.out_classes = out_classes; a.out_counts = out_counts;
  if (N) hipLaunchKernelGGL(sn_cell_kernel, dim3((unsigned)(B * C)), dim3(64), (size_t)N * 24, s, a);
  hipLaunchKernelGGL(sn_rank_kernel, dim3(B), dim3(SN_NT), (size_t)N * 8, s, a);
  CTDET_LAUNCH_CHECK();
  return 0;
}
