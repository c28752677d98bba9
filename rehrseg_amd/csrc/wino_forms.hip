// Transform-domain weights of the fp32 Winograd forward / input-gradient kernels in ONE pass over the parameter.
//
// The panel path runs two passes per launch: parameter -> panel wp[T][Npad][Cin] (rehr_pack_weights_f32), panel ->
// wino_ws (wino_weights*_kernel, w22_weights_kernel).  The Winograd kernels read only the second form, so for weights
// that change every step the panel is written to be read once.  This kernel reads the parameter in its torch layout
// (Cout, Cin, KD, KH, KW) or (Cin, Cout, ...), a channel sub-range of either dimension included, and writes what the
// two passes write, bit for bit (the arithmetic is wino_u33 / wino_u22 of wino_shared.h, the one copy).
//
//   block  = 32 destination rows x 32 source channels (one (nt, chunk) pair of the fragment layout) of one
//            (source phase, depth tap)
//   stage  = the 9 (F(2x2,3x3)) or 4 (one F(2x2,2x2) phase) plane taps of the 1024 (row, channel) pairs into LDS, lanes
//            along the parameter's contiguous axis: taps fastest, then whichever of row / channel has the smaller stride
//            (runs of 9 floats every T floats; the other depth taps of the same lines come from L2)
//   write  = thread t of the block owns float t of each 256-float (lane, element) group of the fragment layout:
//            every store instruction of the block is 1 KB contiguous
#include "common.h"
#include "wino_shared.h"

namespace {

enum FormKind { FORM_F33_FRAG = 0, FORM_F33_PLAIN = 1, FORM_F22_FRAG = 2 };

struct FormPart {
  float* up;          // the part's wino_ws
  int npj;            // (source phase, depth tap) pairs: pj = phase * nd + jd
  int nd;             // depth taps
  int doff0, dstep;   // parameter offset of depth tap jd: doff0 + dstep * jd
  int hw[16];         // parameter offset of plane tap g[a][b]: hw[a * 3 + b] / hw[phase * 4 + a * 2 + b]
};
struct FormParams {
  const float* w;
  int64_t sn, sc;     // element (t, n, ci) = w[n * sn + ci * sc + t]
  int inner_ci;       // the channel stride is the smaller one: lanes walk channels before rows
  int A, Cin, Npad, kchunks;
  FormPart part[MAX_PHASES];
};

constexpr int FORM_ROW = 33;   // LDS: [channel 32][row 32 + 1][taps | 1]

template <int KIND>
__global__ __launch_bounds__(256) void wino_forms_kernel(const FormParams p) {
  constexpr int NTAP = KIND == FORM_F22_FRAG ? 4 : 9, TP = NTAP | 1, NX = KIND == FORM_F22_FRAG ? 9 : 16;
  __shared__ float sg[32 * FORM_ROW * TP];
  const FormPart& q = p.part[blockIdx.z];
  const int pj = blockIdx.y;
  if (pj >= q.npj) return;   // block-uniform: the parts of a launch may differ in their depth taps
  const int ph = pj / q.nd, jd = pj - ph * q.nd;
  const int nt = blockIdx.x / p.kchunks, chunk = blockIdx.x - nt * p.kchunks;
  const int tid = threadIdx.x;
  const int64_t toff = (int64_t)q.doff0 + (int64_t)q.dstep * jd;
  const int hw0 = KIND == FORM_F22_FRAG ? ph * 4 : 0;

  // (the tap table through LDS: a lane-indexed read of the kernel arguments would be a global load in front of every
  // parameter load.  Both loops fully unrolled: all 4 * NTAP loads of a thread are in flight before the first LDS write --
  // small layers are a handful of blocks, and one load per round trip made every launch take 30 us)
  __shared__ int shw[16];
  if (tid < 16) shw[tid] = q.hw[tid];
  __syncthreads();
  float v[4 * NTAP];
#pragma unroll
  for (int i = 0; i < 4 * NTAP; ++i) {
    const int s = i * 256 + tid;
    const int it = s / NTAP, j = s - it * NTAP;
    const int in = it & 31, out = it >> 5;
    const int n = nt * 32 + (p.inner_ci ? out : in), ci = chunk * 32 + (p.inner_ci ? in : out);
    v[i] = 0.f;
    if (n < p.A && ci < p.Cin) v[i] = p.w[(int64_t)n * p.sn + (int64_t)ci * p.sc + toff + shw[hw0 + j]];
  }
#pragma unroll
  for (int i = 0; i < 4 * NTAP; ++i) {
    const int s = i * 256 + tid;
    const int it = s / NTAP, j = s - it * NTAP;
    const int in = it & 31, out = it >> 5;
    const int n_l = p.inner_ci ? out : in, ci_l = p.inner_ci ? in : out;
    sg[(ci_l * FORM_ROW + n_l) * TP + j] = v[i];
  }
  __syncthreads();

#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int n_l, ci_l;
    if (KIND == FORM_F33_PLAIN) {   // U[jd][xi][Npad][Cin]: lanes along the channels
      n_l = k * 8 + (tid >> 5);
      ci_l = tid & 31;
    } else {                        // fragment order: float tid of k-group k = (lane = half * 32 + col, element e)
      const int lane = tid >> 2, e = tid & 3;
      n_l = lane & 31;
      ci_l = k * 8 + (lane >> 5) * 4 + e;
    }
    const float* gp = sg + (ci_l * FORM_ROW + n_l) * TP;
    float u[NX];
    if constexpr (KIND == FORM_F22_FRAG) {
      float g[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) g[a][b] = gp[a * 2 + b];
      wino_u22(g, u);
    } else {
      float g[3][3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) g[a][b] = gp[a * 3 + b];
      wino_u33(g, u);
    }
    if (KIND == FORM_F33_PLAIN) {
      const int n = nt * 32 + n_l, ci = chunk * 32 + ci_l;
      const int64_t per = (int64_t)p.Npad * p.Cin;
      if (ci < p.Cin) {
        float* o = q.up + (int64_t)jd * 16 * per + (int64_t)n * p.Cin + ci;
#pragma unroll
        for (int x = 0; x < NX; ++x) o[x * per] = u[x];
      }
    } else {
      const int64_t xs = (int64_t)(p.Npad / 32) * p.kchunks * 1024;   // floats per transformed tap
      float* o = q.up + (int64_t)pj * NX * xs + ((int64_t)nt * p.kchunks + chunk) * 1024 + k * 256 + tid;
#pragma unroll
      for (int x = 0; x < NX; ++x) o[x * xs] = u[x];
    }
  }
}

FormKind form_kind(WinoRoute r) {
  return r >= WINO_FLAT22 ? FORM_F22_FRAG : r == WINO_SMALL ? FORM_F33_PLAIN : FORM_F33_FRAG;
}

// the taps of one part as parameter offsets; the planners have admitted the taps (three_taps / plan_axis)
bool fill_part(FormKind kind, const rehr_gather_gemm_desc& d, FormPart& q) {
  const int khw = d.KH * d.KW;
  q.up = d.wino_ws;
  q.nd = d.td.count;
  q.doff0 = d.td.k0 * khw;
  q.dstep = d.td.ks * khw;
  for (int i = 0; i < 16; ++i) q.hw[i] = 0;
  if (kind == FORM_F22_FRAG) {
    AxisPlan ah, aw;
    if (!plan_axis(d.th, d.sh, d.bh, ah) || !plan_axis(d.tw, d.sw, d.bw, aw) || ah.nph * aw.nph > WINO_MAXPH) return false;
    q.npj = ah.nph * aw.nph * d.td.count;
    for (int p_h = 0; p_h < ah.nph; ++p_h)
      for (int p_w = 0; p_w < aw.nph; ++p_w)
        for (int a = 0; a < 2; ++a)
          for (int b = 0; b < 2; ++b)
            q.hw[(p_h * aw.nph + p_w) * 4 + a * 2 + b] = ah.kidx[p_h][a] * d.KW + aw.kidx[p_w][b];
    return true;
  }
  if (d.th.count != 3 || d.tw.count != 3) return false;
  q.npj = d.td.count;
  bool seen[9] = {false};
  for (int jh = 0; jh < 3; ++jh)
    for (int jw = 0; jw < 3; ++jw) {
      const int a = d.bh + d.th.off0 + d.th.offs * jh + 1;   // source offset + 1 in {0, 1, 2}
      const int b = d.bw + d.tw.off0 + d.tw.offs * jw + 1;
      if (a < 0 || a > 2 || b < 0 || b > 2) return false;
      q.hw[a * 3 + b] = (d.th.k0 + d.th.ks * jh) * d.KW + (d.tw.k0 + d.tw.ks * jw);
      seen[a * 3 + b] = true;
    }
  for (int i = 0; i < 9; ++i)
    if (!seen[i]) return false;
  return true;
}

template <int KIND>
void launch_forms(const FormParams& p, int parts, int max_pj, hipStream_t stream) {
  dim3 grid((unsigned)((p.Npad / 32) * p.kchunks), (unsigned)max_pj, (unsigned)parts);
  hipLaunchKernelGGL(wino_forms_kernel<KIND>, grid, dim3(256), 0, stream, p);
}

}  // namespace

// Parts of the same kind and channel geometry share a launch (blockIdx.z = part): the output phases of a transposed
// convolution, the depth-tap ranges of a split.
int wino_forms_launch(const WinoRoute* r, const rehr_gather_gemm_desc* ds, int count, const WinoWeightSrc& src,
                      hipStream_t stream) {
  if (count < 1 || count > MAX_PHASES) return REHR_EINVAL;
  bool done[MAX_PHASES] = {false};
  FormPart parts[MAX_PHASES];
  for (int i = 0; i < count; ++i) {
    if (r[i] == WINO_NONE) return REHR_ENOSUP;
    if (!fill_part(form_kind(r[i]), ds[i], parts[i]) || parts[i].npj < 1 || parts[i].npj > 65535) return REHR_EINVAL;
  }
  for (int i = 0; i < count; ++i) {
    if (done[i]) continue;
    const FormKind kind = form_kind(r[i]);
    FormParams p;
    p.w = src.w;
    p.sn = src.sn;
    p.sc = src.sc;
    p.inner_ci = src.sc < src.sn ? 1 : 0;
    p.A = ds[i].Cout;
    p.Cin = ds[i].Cin;
    p.Npad = ds[i].Npad;
    p.kchunks = (ds[i].Cin + 31) / 32;
    int n = 0, max_pj = 0;
    for (int j = i; j < count; ++j) {
      if (done[j] || form_kind(r[j]) != kind || ds[j].Cout != p.A || ds[j].Cin != p.Cin || ds[j].Npad != p.Npad) continue;
      done[j] = true;
      p.part[n++] = parts[j];
      if (parts[j].npj > max_pj) max_pj = parts[j].npj;
    }
    for (int j = n; j < MAX_PHASES; ++j) p.part[j] = p.part[0];
    if (kind == FORM_F22_FRAG) launch_forms<FORM_F22_FRAG>(p, n, max_pj, stream);
    else if (kind == FORM_F33_PLAIN) launch_forms<FORM_F33_PLAIN>(p, n, max_pj, stream);
    else launch_forms<FORM_F33_FRAG>(p, n, max_pj, stream);
    REHR_LAUNCH_CHECK();
  }
  return REHR_OK;
}
