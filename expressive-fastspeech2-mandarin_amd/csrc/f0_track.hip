// F0 tracking over the YIN table (include/fs2hip_f0_track.h): per frame the troughs of the dp row
// as weighted candidates (one wave per frame, ballots and a wave scan), then per utterance a
// Viterbi recursion over pitch bin and voicing (one workgroup, lane n = bin n in both voicings,
// delta double-buffered in LDS, one barrier per frame) and its back-trace. The device compares,
// adds and looks up; every logarithm lives in the caller's tables. No atomics.
#include "f0_track_sizes.h"
#include "fs2_common.h"
#include "fs2hip_f0_track.h"

// Nothing here may be contracted: the refinement is the one of fs2hip_f0.h, operation by operation.
#pragma clang fp contract(off)

namespace {

constexpr int kNT = 256;                      // threads of the recursion's workgroup: one per bin
constexpr int kT1 = FS2_F0_TRACK_THR + 1;     // side of lm0 / lm1; also "no threshold": a = 101
constexpr int kCapMax = FS2_F0_TRACK_CAP_MAX;
constexpr int kTB = FS2_F0_TRACK_TB;

__device__ __forceinline__ double neg_inf() { return -__builtin_inf(); }

// frames of utterance b
__device__ __forceinline__ int ft_frames(const int64_t *lens, int b, int hop, int F_max) {
  if (lens == nullptr) return F_max;
  int64_t n = lens[b];
  if (n < 0) n = 0;
  const int64_t F = n / hop + 1;
  return F > F_max ? F_max : (int)F;
}

// ------------------------------------------------------------------------------------------------
// observations: one wave (one workgroup of 64) per (utterance, frame)

struct ObsArgs {
  const double *cmnd;
  const int64_t *lens;
  int F_max, hop, tau_min, tau_max, N, cap;
  double sr, f0_floor, f0_ceil;
  const double *thr, *lm0, *lm1, *edges;
  int *head;
  double *lm, *fq;
  int *bin;
};

struct Cand {
  bool keep;
  double d, p, f;
};

// the candidate at lag t, if dp has a trough there and its refined f is in range
__device__ __forceinline__ Cand ft_cand(const double *__restrict__ row, int t, const ObsArgs &A) {
  Cand c;
  c.keep = false;
  c.d = c.p = c.f = 0.0;
  if (t < A.tau_max) {
    const double a = row[t - 1], b = row[t], cc = row[t + 1];
    if (b < a && b <= cc) {
      const double den = (a - 2.0 * b) + cc;
      const double delta = den > 0.0 ? (0.5 * (a - cc)) / den : 0.0;
      c.p = (double)t + delta;
      c.f = A.sr / c.p;
      c.d = b;
      c.keep = A.f0_floor <= c.f && c.f <= A.f0_ceil;
    }
  }
  return c;
}

// a: the smallest i in 1 .. 100 with d < thr[i], 101 when there is none
__device__ __forceinline__ int ft_thr_index(const double *__restrict__ thr, double d) {
  int lo = 1, hi = kT1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (d < thr[mid])
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// the number of n in 1 .. N - 1 with p <= edges[n] (edges decrease)
__device__ __forceinline__ int ft_bin(const double *__restrict__ edges, int N, double p) {
  int lo = 0, hi = N - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p <= edges[mid])
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(FS2_WAVE) void f0_track_obs_kernel(ObsArgs A) {
  __shared__ double s_lm[kCapMax], s_f[kCapMax];
  __shared__ int s_bin[kCapMax];
  const int lane = threadIdx.x, k = blockIdx.x, b = blockIdx.y;
  if (k >= ft_frames(A.lens, b, A.hop, A.F_max)) return;  // uniform
  const int64_t fr = (int64_t)b * A.F_max + k;
  const double *row = A.cmnd + fr * (A.tau_max + 1);
  int *head = A.head + fr * 2;

  // the best: the smallest dp among the kept candidates, the smaller lag among equals
  double bd = __builtin_inf();
  int bt = INT32_MAX;
  for (int base = A.tau_min; base < A.tau_max; base += FS2_WAVE) {
    const int t = base + lane;
    const Cand c = ft_cand(row, t, A);
    if (c.keep && c.d < bd) {  // a lane's lags ascend: < keeps its smaller one
      bd = c.d;
      bt = t;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(bd, o, FS2_WAVE);
    const int ot = __shfl_xor(bt, o, FS2_WAVE);
    if (ot != INT32_MAX && (bt == INT32_MAX || od < bd || (od == bd && ot < bt))) {
      bd = od;
      bt = ot;
    }
  }
  if (bt == INT32_MAX) {  // uniform: no candidate
    if (lane == 0) {
      head[0] = kT1;
      head[1] = 0;
    }
    return;
  }

  // the masses, in lag order: m is the running minimum of a over the kept candidates before
  int carry = kT1, count = 0;
  for (int base = A.tau_min; base < A.tau_max; base += FS2_WAVE) {
    const int t = base + lane;
    const Cand c = ft_cand(row, t, A);
    const int a = c.keep ? ft_thr_index(A.thr, c.d) : kT1;
    int inc = a;
#pragma unroll
    for (int d = 1; d < FS2_WAVE; d <<= 1) {
      const int v = __shfl_up(inc, d, FS2_WAVE);
      if (lane >= d) inc = min(inc, v);
    }
    int exc = __shfl_up(inc, 1, FS2_WAVE);
    if (lane == 0) exc = kT1;
    const int m = min(carry, exc);
    carry = min(carry, __shfl(inc, FS2_WAVE - 1, FS2_WAVE));
    double lm = neg_inf();
    if (c.keep) {
      const int u = a - 1, v = m - 1;
      if (t == bt)
        lm = A.lm1[u * kT1 + v];  // v >= u: a of the best is the smallest
      else if (a < m)
        lm = A.lm0[u * kT1 + v];
    }
    const bool has = c.keep && lm > neg_inf();
    const unsigned long long mask = __ballot(has);
    const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
    if (has && pos < kCapMax) {
      s_lm[pos] = lm;
      s_f[pos] = c.f;
      s_bin[pos] = ft_bin(A.edges, A.N, c.p);
    }
    count += __popcll(mask);
  }
  count = min(count, kCapMax);
  __syncthreads();  // one wave: the list is written

  // one candidate per bin: the larger log-mass, the earlier one among equals
  const int64_t e0 = fr * A.cap;
  int kept = 0;
  for (int base = 0; base < count; base += FS2_WAVE) {
    const int i = base + lane;
    bool stay = i < count;
    if (stay) {
      const int bi = s_bin[i];
      const double li = s_lm[i];
      for (int j = 0; j < count; ++j) {
        const double lj = s_lm[j];
        if (j != i && s_bin[j] == bi && (lj > li || (lj == li && j < i))) stay = false;
      }
    }
    const unsigned long long mask = __ballot(stay);
    const int pos = kept + __popcll(mask & ((1ull << lane) - 1ull));
    if (stay && pos < A.cap) {
      A.lm[e0 + pos] = s_lm[i];
      A.fq[e0 + pos] = s_f[i];
      A.bin[e0 + pos] = s_bin[i];
    }
    kept += __popcll(mask);
  }
  if (lane == 0) {
    head[0] = ft_thr_index(A.thr, bd) - 1;
    head[1] = min(kept, A.cap);
  }
}

// ------------------------------------------------------------------------------------------------
// the recursion and the back-trace: one workgroup per utterance

struct VitArgs {
  const int64_t *lens;
  int F_max, hop, N, K, cap;
  const int *head;
  const double *lm, *fq;
  const int *bin;
  const double *lu, *ts, *tx;
  double log_floor, log_init;
  unsigned char *bp;
  double *f0;
  int *state;
  double *score;
};

// What the recursion holds of a frame ahead of its turn: the head, and list entry tid.
struct Pre {
  int g, cnt, bin;
  double lm;
};

// LDS writes done, then the barrier: the global loads and stores in flight stay in flight.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

template <int KT>
__global__ __launch_bounds__(kNT) void f0_track_viterbi_kernel(VitArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int N = A.N, K = KT > 0 ? KT : A.K, NP = (int)ft_row(N, K);
  // buffer i: voiced row at lds + 2 i NP, unvoiced row NP after it; bin n at slot K + n
  double *ob = lds + 4 * NP;  // voiced observations of two frames, [2][N]
  unsigned char *stage = reinterpret_cast<unsigned char *>(lds + 4 * NP + 2 * N);
  const int F_b = ft_frames(A.lens, b, A.hop, A.F_max);
  const int64_t fr0 = (int64_t)b * A.F_max;
  const int *head = A.head + fr0 * 2;
  unsigned char *bp = A.bp + fr0 * 2 * N;
  double *f0o = A.f0 + fr0;
  int *sto = A.state + fr0;

  constexpr int KR = KT > 0 ? KT : 1;
  double ts[KR + 1], tx[KR + 1];
  if (KT > 0) {
#pragma unroll
    for (int d = 0; d <= KR; ++d) {
      ts[d] = A.ts[d];
      tx[d] = A.tx[d];
      asm volatile("" : "+v"(ts[d]), "+v"(tx[d]));  // in vector registers: 52 scalar ones would spill
    }
  }

  for (int i = tid; i < 4 * NP; i += kNT) lds[i] = neg_inf();
  for (int i = tid; i < 2 * N; i += kNT) ob[i] = A.log_floor;

  auto fetch = [&](int k) {
    Pre p;
    p.g = kT1;
    p.cnt = 0;
    p.bin = 0;
    p.lm = 0.0;
    if (k < F_b) {
      p.g = head[2 * k];
      p.cnt = head[2 * k + 1];
      if (tid < A.cap) {
        const int64_t e = (fr0 + k) * A.cap + tid;
        p.bin = A.bin[e];
        p.lm = A.lm[e];
      }
    }
    return p;
  };
  auto scatter = [&](const Pre &p, int buf) {
    if (tid < p.cnt && tid < A.cap && (unsigned)p.bin < (unsigned)N) ob[buf * N + p.bin] = p.lm;
  };
  auto lu_of = [&](const Pre &p) { return A.lu[p.g < 0 ? 0 : (p.g > kT1 ? kT1 : p.g)]; };

  Pre p = fetch(0);
  __syncthreads();  // the rows and the observation slots are set
  scatter(p, 0);
  double lu_cur = lu_of(p), lu_next;
  p = fetch(1);
  __syncthreads();

  // frame 0
  if (tid < N) {
    const double o = ob[tid];
    ob[tid] = A.log_floor;
    lds[K + tid] = o + A.log_init;
    lds[NP + K + tid] = lu_cur + A.log_init;
  }
  scatter(p, 1);
  lu_next = lu_of(p);
  p = fetch(2);
  lds_barrier();

  for (int k = 1; k < F_b; ++k) {
    const int cur = k & 1;
    lu_cur = lu_next;
    double o = 0.0;
    if (tid < N) {
      o = ob[cur * N + tid];
      ob[cur * N + tid] = A.log_floor;  // for frame k + 2, scattered after the barrier below
    }
    scatter(p, cur ^ 1);  // frame k + 1: its slots were reset in frame k - 1
    lu_next = lu_of(p);
    p = fetch(k + 2);
    if (tid < N) {
      const double *pv = lds + (cur ^ 1) * 2 * NP + K + tid, *pu = pv + NP;
      double bv = neg_inf(), bu = neg_inf();
      int cv = 0, cu = 0;
#pragma unroll
      for (int off = -K; off <= K; ++off) {  // predecessor bin tid + off: -inf outside 0 .. N - 1
        const int a = off < 0 ? -off : off;
        const double s = KT > 0 ? ts[a <= KR ? a : 0] : A.ts[a], x = KT > 0 ? tx[a <= KR ? a : 0] : A.tx[a];
        const double dv = pv[off], du = pu[off];
        const int code = (off + K) * 2;
        const double v0 = dv + s, v1 = du + x, u0 = du + s, u1 = dv + x;
        if (v0 > bv) {
          bv = v0;
          cv = code;
        }
        if (v1 > bv) {
          bv = v1;
          cv = code + 1;
        }
        if (u0 > bu) {
          bu = u0;
          cu = code;
        }
        if (u1 > bu) {
          bu = u1;
          cu = code + 1;
        }
      }
      double *cvr = lds + cur * 2 * NP + K + tid;
      cvr[0] = o + bv;
      cvr[NP] = lu_cur + bu;
      unsigned char *row = bp + (int64_t)k * 2 * N;
      row[tid] = (unsigned char)cv;
      row[N + tid] = (unsigned char)cu;
    }
    lds_barrier();
  }

  // the final state: the largest delta, the lowest index among equals; wave 0, then lane 0
  const double *fin = lds + ((F_b - 1) & 1) * 2 * NP + K;
  int *ctl = reinterpret_cast<int *>(ob);  // ob is dead: [0] the state the back-trace hands on
  if (tid < FS2_WAVE) {
    double bd = neg_inf();
    int bs = INT32_MAX;
    for (int s = tid; s < 2 * N; s += FS2_WAVE) {  // ascending per lane: > keeps the lower index
      const double v = s < N ? fin[s] : fin[NP + s - N];
      if (bs == INT32_MAX || v > bd) {
        bd = v;
        bs = s;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double od = __shfl_xor(bd, o, FS2_WAVE);
      const int os = __shfl_xor(bs, o, FS2_WAVE);
      if (os != INT32_MAX && (bs == INT32_MAX || od > bd || (od == bd && os < bs))) {
        bd = od;
        bs = os;
      }
    }
    if (tid == 0) {
      ctl[0] = bs;
      if (A.score != nullptr) A.score[b] = bd;
    }
  }
  __threadfence();  // the predecessor bytes, before other threads read them back
  __syncthreads();

  // Back-trace, kTB frames at a time from the end: every thread stages their predecessor bytes in
  // LDS (at the source's alignment, so that the middle goes as 32-bit words), lane 0 walks them and
  // leaves the state index of each frame in the state output, which the last step below rewrites.
  for (int hi = F_b - 1; hi >= 1; hi -= kTB) {
    const int lo = hi - kTB + 1 > 1 ? hi - kTB + 1 : 1;
    const unsigned char *src = bp + (int64_t)lo * 2 * N;
    const int len = (hi - lo + 1) * 2 * N;
    const int mis = (int)(reinterpret_cast<uintptr_t>(src) & 3);
    unsigned char *dst = stage + mis;  // stage is 8-byte aligned
    const int headb = mis ? min(4 - mis, len) : 0;
    const int words = (len - headb) >> 2, tail0 = headb + words * 4;
    if (tid < headb) dst[tid] = src[tid];
    for (int w = tid; w < words; w += kNT)
      reinterpret_cast<unsigned *>(dst + headb)[w] = reinterpret_cast<const unsigned *>(src + headb)[w];
    if (tid < len - tail0) dst[tail0 + tid] = src[tail0 + tid];
    __syncthreads();
    if (tid == 0) {
      int s = ctl[0];
      for (int k = hi; k >= lo; --k) {
        sto[k] = s;
        const bool voiced = s < N;
        const int n = voiced ? s : s - N;
        const int code = dst[(k - lo) * 2 * N + s];
        int pn = n + (code >> 1) - K;
        pn = pn < 0 ? 0 : (pn > N - 1 ? N - 1 : pn);  // a stored code never leaves the bins
        const bool pvoiced = (code & 1) ? !voiced : voiced;
        s = pvoiced ? pn : N + pn;
      }
      ctl[0] = s;
    }
    __syncthreads();
  }
  if (tid == 0) {
    sto[0] = ctl[0];
    __threadfence();  // the state indices, before the other threads read them
  }
  __syncthreads();

  // f0 and state of every frame: the candidate in the path's bin, if the frame has one
  for (int k = tid; k < A.F_max; k += kNT) {
    double f = 0.0;
    int st = -1;
    if (k < F_b) {
      const int s = sto[k];
      if (s < N) {
        const int cnt = min(head[2 * k + 1], A.cap);
        const int64_t e0 = (fr0 + k) * A.cap;
        for (int j = 0; j < cnt; ++j)
          if (A.bin[e0 + j] == s) {
            f = A.fq[e0 + j];
            st = s;
          }
      }
    }
    f0o[k] = f;
    sto[k] = st;
  }
}

}  // namespace

extern "C" int64_t fs2_f0_track_lds_bytes(int n_bins, int max_step) {
  return n_bins < 1 || max_step < 0 ? 0 : f0_track_lds_bytes(n_bins, max_step);
}

extern "C" int64_t fs2_f0_track_workspace_bytes(int B, int F_max, int tau_min, int tau_max, int n_bins) {
  if (B < 1 || F_max < 1 || n_bins < 1 || tau_min < 2 || tau_min >= tau_max) return 0;
  return f0_track_sizes(B, F_max, tau_min, tau_max, n_bins).bytes;
}

extern "C" int fs2_f0_track(const double *cmnd, const int64_t *lens, int B, int F_max, int hop, double sr, int tau_min,
                            int tau_max, double f0_floor, double f0_ceil, const double *thr, const double *lm0,
                            const double *lm1, const double *lu, const double *edges, int n_bins,
                            const double *trans_same, const double *trans_switch, int max_step, double log_floor,
                            double log_init, void *workspace, int64_t ws_bytes, double *f0, int32_t *state,
                            double *score, fs2_stream_t stream) {
  if (cmnd == nullptr || thr == nullptr || lm0 == nullptr || lm1 == nullptr || lu == nullptr || edges == nullptr ||
      trans_same == nullptr || trans_switch == nullptr || workspace == nullptr || f0 == nullptr || state == nullptr)
    return FS2_EINVAL;
  if (B < 1 || F_max < 1 || hop < 1 || n_bins < 1 || max_step < 0 || !(sr > 0.0)) return FS2_EINVAL;
  if (tau_min < 2 || tau_min >= tau_max) return FS2_EINVAL;
  if (B > 65535 || n_bins > FS2_F0_TRACK_BINS_MAX || max_step > FS2_F0_TRACK_STEP_MAX) return FS2_EUNSUPPORTED;
  const int64_t lds = f0_track_lds_bytes(n_bins, max_step);
  if (lds > FS2_F0_TRACK_LDS_BYTES) return FS2_EUNSUPPORTED;
  const F0TrackSizes sz = f0_track_sizes(B, F_max, tau_min, tau_max, n_bins);
  int64_t widest = (int64_t)tau_max + 1;
  if (2 * (int64_t)n_bins > widest) widest = 2 * (int64_t)n_bins;
  if (sz.cap > widest) widest = sz.cap;
  if (ft_sat_mul(ft_sat_mul(B, F_max), widest) > ((int64_t)1 << 40)) return FS2_EUNSUPPORTED;
  if (ws_bytes < sz.bytes || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return FS2_EINVAL;
  char *ws = static_cast<char *>(workspace);
  const hipStream_t s = as_stream(stream);

  ObsArgs o;
  o.cmnd = cmnd;
  o.lens = lens;
  o.F_max = F_max;
  o.hop = hop;
  o.tau_min = tau_min;
  o.tau_max = tau_max;
  o.N = n_bins;
  o.cap = (int)sz.cap;
  o.sr = sr;
  o.f0_floor = f0_floor;
  o.f0_ceil = f0_ceil;
  o.thr = thr;
  o.lm0 = lm0;
  o.lm1 = lm1;
  o.edges = edges;
  o.head = reinterpret_cast<int *>(ws + sz.head);
  o.lm = reinterpret_cast<double *>(ws + sz.lm);
  o.fq = reinterpret_cast<double *>(ws + sz.fq);
  o.bin = reinterpret_cast<int *>(ws + sz.bin);
  // frames on x: F_max has no 65535 limit there
  hipLaunchKernelGGL(f0_track_obs_kernel, dim3((unsigned)F_max, (unsigned)B), dim3(FS2_WAVE), 0, s, o);
  FS2_CHECK_LAUNCH();

  VitArgs v;
  v.lens = lens;
  v.F_max = F_max;
  v.hop = hop;
  v.N = n_bins;
  v.K = max_step;
  v.cap = (int)sz.cap;
  v.head = o.head;
  v.lm = o.lm;
  v.fq = o.fq;
  v.bin = o.bin;
  v.lu = lu;
  v.ts = trans_same;
  v.tx = trans_switch;
  v.log_floor = log_floor;
  v.log_init = log_init;
  v.bp = reinterpret_cast<unsigned char *>(ws + sz.bp);
  v.f0 = f0;
  v.state = state;
  v.score = score;
  if (max_step == 12)
    hipLaunchKernelGGL(f0_track_viterbi_kernel<12>, dim3((unsigned)B), dim3(kNT), (size_t)lds, s, v);
  else
    hipLaunchKernelGGL(f0_track_viterbi_kernel<0>, dim3((unsigned)B), dim3(kNT), (size_t)lds, s, v);
  FS2_CHECK_LAUNCH();
  return FS2_OK;
}
