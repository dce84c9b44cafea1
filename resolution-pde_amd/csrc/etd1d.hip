// Exponential-time-differencing generator for u_t = L u - (c/2) (u^2)_x on a periodic 1-D domain (Burgers,
// Kuramoto-Sivashinsky; data_generation/burgers_1d.py, ks_1d.py).  ETDRK4 in the Kassam-Trefethen form,
// pseudo-spectral.  gfx950, wave64.
//
// The state is the half spectrum v = rfft(u), [B][re|im][kp] (halfspec.h, M = 1).  With Nhat(w) = i g rfft(irfft(w)^2) one step is
//   Nv = Nhat(v), a = E2 v + Q Nv;   Na = Nhat(a), b = E2 v + Q Na;   Nb = Nhat(b), c = E2 a + Q (2 Nb - Nv);
//   Nc = Nhat(c), v <- E v + f1 Nv + 2 f2 (Na + Nb) + f3 Nc
// and sixteen launches on the caller's stream, four per stage, no host synchronisation:
//   synthesis        irfft of the stage's spectrum (v, a, b, c) to [B][N]
//   k_etd_square     u -> u^2 in place
//   analysis         F = rfft(u^2)
//   k_etd_stage<S>   i g F in registers (a swap and a sign) and the stage's update, fused multiply-adds only
// The seven tables (E, E2, Q, f1, f2, f3, g) [kp] are formed by the caller in float64 and rounded to fp32 once
// (include/rpde.h has the formulas): no division and no transcendental here.  The transforms are the one-dimensional
// case of the full-spectrum real DFT of cf_dft.h (hs_rfft / hs_irfft at M = 1: no column plan, GEMM form; 1 / N in the
// synthesis table; the rfft / irfft entries and the random field are in halfspec.hip).  The stage kernels stream as ns_solver.hip does: a thread owns one 16-byte group of k for both re
// and im, every load and store is a whole float4, grid (blocks, B).  The square is not folded into a transform: the
// GEMMs carry no squaring prologue, and one more epilogue there would serve this file alone.
// The stage sequence is a pure function of v: k calls of n steps give the bits of one call of k n steps.  No atomics
// anywhere: identical calls give identical bits.
// rpde_etd1d_steps_cx is the same step for a symbol with odd derivatives, l_n += i (c1 kappa_n + c3 kappa_n^3) (advection,
// dispersion: Korteweg-de Vries, data_generation/kdv_1d.py): E, E2, Q, f1, f2, f3 are complex [re|im][kp], g stays real,
// and the stage kernels are k_etd_stage_cx<S>.  The same workspace, launches and transforms; k_etd_stage<S> and the
// real call are as they were.
#include "etd_cx.h"
#include "halfspec.h"

namespace rpde {

struct EtdTables { const float *E, *E2, *Q, *f1, *f2, *f3, *g; };
// v: the state; nv: Nv; a: stage a; sum: Na, then Na + Nb; bc: stage b, then stage c (each the next synthesis' input)
struct EtdBufs { float *v, *nv, *a, *sum, *bc; };

// Stage S of one step from the raw product spectrum F = rfft(w^2), w the stage's field:
//   S = 0   Nv = i g F           stores Nv and a = E2 v + Q Nv
//   S = 1   Na = i g F           stores sum = Na and b = E2 v + Q Na
//   S = 2   Nb = i g F           stores sum += Nb and c = E2 a + Q (2 Nb - Nv)
//   S = 3   Nc = i g F           v <- E v + f1 Nv + 2 f2 sum + f3 Nc, in place
// i g (Fr + i Fi) = -g Fi + i g Fr.  grid (blocks, B).  Padded columns (k > N/2) are written as zeros: the synthesis
// reads them.
template <int S>
__global__ __launch_bounds__(256) void k_etd_stage(EtdBufs u, const float* __restrict__ F, EtdTables t, HalfSpec g) {
  const long per = 2L * g.kp, base = (long)blockIdx.y * per;
  const float* __restrict__ Fb = F + base;
  const int c4n = g.kp / 4;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < c4n; q += gridDim.x * blockDim.x) {
    const int k0 = q * 4;
    const long ore = base + k0, oim = ore + g.kp;
    float fr[4], fi[4], gg[4], nr[4], ni[4];
    ld4(Fb + k0, fr);
    ld4(Fb + g.kp + k0, fi);
    ld4(t.g + k0, gg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nr[j] = -gg[j] * fi[j];
      ni[j] = gg[j] * fr[j];
    }
    if (S == 0 || S == 1) {
      float vr[4], vi[4], e2[4], qq[4], orr[4], oi[4];
      ld4(u.v + ore, vr); ld4(u.v + oim, vi);
      ld4(t.E2 + k0, e2); ld4(t.Q + k0, qq);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = k0 + j < g.K;
        orr[j] = live ? fmaf(e2[j], vr[j], qq[j] * nr[j]) : 0.f;
        oi[j] = live ? fmaf(e2[j], vi[j], qq[j] * ni[j]) : 0.f;
        nr[j] = live ? nr[j] : 0.f;
        ni[j] = live ? ni[j] : 0.f;
      }
      float* __restrict__ nout = S == 0 ? u.nv : u.sum;
      float* __restrict__ sout = S == 0 ? u.a : u.bc;
      st4(nout + ore, nr); st4(nout + oim, ni);
      st4(sout + ore, orr); st4(sout + oim, oi);
    } else if (S == 2) {
      float ar[4], ai[4], pr[4], pi[4], sr[4], si[4], e2[4], qq[4], cr[4], ci[4];
      ld4(u.a + ore, ar);   ld4(u.a + oim, ai);
      ld4(u.nv + ore, pr);  ld4(u.nv + oim, pi);
      ld4(u.sum + ore, sr); ld4(u.sum + oim, si);
      ld4(t.E2 + k0, e2);   ld4(t.Q + k0, qq);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = k0 + j < g.K;
        cr[j] = live ? fmaf(e2[j], ar[j], qq[j] * fmaf(2.f, nr[j], -pr[j])) : 0.f;
        ci[j] = live ? fmaf(e2[j], ai[j], qq[j] * fmaf(2.f, ni[j], -pi[j])) : 0.f;
        sr[j] = live ? sr[j] + nr[j] : 0.f;
        si[j] = live ? si[j] + ni[j] : 0.f;
      }
      st4(u.sum + ore, sr); st4(u.sum + oim, si);
      st4(u.bc + ore, cr);  st4(u.bc + oim, ci);
    } else {
      float vr[4], vi[4], pr[4], pi[4], sr[4], si[4], e[4], c1[4], c2[4], c3[4];
      ld4(u.v + ore, vr);   ld4(u.v + oim, vi);
      ld4(u.nv + ore, pr);  ld4(u.nv + oim, pi);
      ld4(u.sum + ore, sr); ld4(u.sum + oim, si);
      ld4(t.E + k0, e);     ld4(t.f1 + k0, c1);
      ld4(t.f2 + k0, c2);   ld4(t.f3 + k0, c3);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = k0 + j < g.K;
        const float two_f2 = 2.f * c2[j];
        vr[j] = live ? fmaf(e[j], vr[j], fmaf(c1[j], pr[j], fmaf(two_f2, sr[j], c3[j] * nr[j]))) : 0.f;
        vi[j] = live ? fmaf(e[j], vi[j], fmaf(c1[j], pi[j], fmaf(two_f2, si[j], c3[j] * ni[j]))) : 0.f;
      }
      st4(u.v + ore, vr); st4(u.v + oim, vi);
    }
  }
}

// k_etd_stage for complex tables (rpde_etd1d_steps_cx: a symbol with odd derivatives): E, E2, Q, f1, f2, f3 are
// [re|im][kp], the plane layout of the spectra, g stays real.  Every coefficient product of k_etd_stage becomes a complex
// one -- the real plane's multiply or fma, then two more fmas with the imaginary plane -- in the same order of terms.
// Same geometry, same streaming: the imaginary planes are further whole float4 loads, all of them unconditional.  The
// masked values are formed before the selects: a select whose arm holds the only use of a load becomes a branch with
// that element's load inside it, which splits the float4 and waits per element.  etd_cmul / etd_cfma: etd_cx.h.
template <int S>
__global__ __launch_bounds__(256) void k_etd_stage_cx(EtdBufs u, const float* __restrict__ F, EtdTables t, HalfSpec g) {
  const long per = 2L * g.kp, base = (long)blockIdx.y * per;
  const float* __restrict__ Fb = F + base;
  const int c4n = g.kp / 4;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < c4n; q += gridDim.x * blockDim.x) {
    const int k0 = q * 4, k1 = k0 + g.kp;                     // a table's real and imaginary group
    const long ore = base + k0, oim = ore + g.kp;
    float fr[4], fi[4], gg[4], nr[4], ni[4];
    ld4(Fb + k0, fr);
    ld4(Fb + k1, fi);
    ld4(t.g + k0, gg);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nr[j] = -gg[j] * fi[j];
      ni[j] = gg[j] * fr[j];
    }
    if (S == 0 || S == 1) {
      float vr[4], vi[4], e2r[4], e2i[4], qr[4], qi[4], orr[4], oi[4];
      ld4(u.v + ore, vr);   ld4(u.v + oim, vi);
      ld4(t.E2 + k0, e2r);  ld4(t.E2 + k1, e2i);
      ld4(t.Q + k0, qr);    ld4(t.Q + k1, qi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = k0 + j < g.K;
        float xr, xi;
        etd_cmul(qr[j], qi[j], nr[j], ni[j], xr, xi);
        etd_cfma(e2r[j], e2i[j], vr[j], vi[j], xr, xi);
        orr[j] = live ? xr : 0.f;
        oi[j] = live ? xi : 0.f;
        nr[j] = live ? nr[j] : 0.f;
        ni[j] = live ? ni[j] : 0.f;
      }
      float* __restrict__ nout = S == 0 ? u.nv : u.sum;
      float* __restrict__ sout = S == 0 ? u.a : u.bc;
      st4(nout + ore, nr); st4(nout + oim, ni);
      st4(sout + ore, orr); st4(sout + oim, oi);
    } else if (S == 2) {
      float ar[4], ai[4], pr[4], pi[4], sr[4], si[4], e2r[4], e2i[4], qr[4], qi[4], cr[4], ci[4];
      ld4(u.a + ore, ar);   ld4(u.a + oim, ai);
      ld4(u.nv + ore, pr);  ld4(u.nv + oim, pi);
      ld4(u.sum + ore, sr); ld4(u.sum + oim, si);
      ld4(t.E2 + k0, e2r);  ld4(t.E2 + k1, e2i);
      ld4(t.Q + k0, qr);    ld4(t.Q + k1, qi);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = k0 + j < g.K;
        float xr, xi;
        etd_cmul(qr[j], qi[j], fmaf(2.f, nr[j], -pr[j]), fmaf(2.f, ni[j], -pi[j]), xr, xi);
        etd_cfma(e2r[j], e2i[j], ar[j], ai[j], xr, xi);
        const float tr = sr[j] + nr[j], ti = si[j] + ni[j];
        cr[j] = live ? xr : 0.f;
        ci[j] = live ? xi : 0.f;
        sr[j] = live ? tr : 0.f;
        si[j] = live ? ti : 0.f;
      }
      st4(u.sum + ore, sr); st4(u.sum + oim, si);
      st4(u.bc + ore, cr);  st4(u.bc + oim, ci);
    } else {
      float vr[4], vi[4], pr[4], pi[4], sr[4], si[4], er[4], ei[4], c1r[4], c1i[4], c2r[4], c2i[4], c3r[4], c3i[4];
      ld4(u.v + ore, vr);   ld4(u.v + oim, vi);
      ld4(u.nv + ore, pr);  ld4(u.nv + oim, pi);
      ld4(u.sum + ore, sr); ld4(u.sum + oim, si);
      ld4(t.E + k0, er);    ld4(t.E + k1, ei);
      ld4(t.f1 + k0, c1r);  ld4(t.f1 + k1, c1i);
      ld4(t.f2 + k0, c2r);  ld4(t.f2 + k1, c2i);
      ld4(t.f3 + k0, c3r);  ld4(t.f3 + k1, c3i);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool live = k0 + j < g.K;
        float xr, xi;
        etd_cmul(c3r[j], c3i[j], nr[j], ni[j], xr, xi);
        etd_cfma(2.f * c2r[j], 2.f * c2i[j], sr[j], si[j], xr, xi);
        etd_cfma(c1r[j], c1i[j], pr[j], pi[j], xr, xi);
        etd_cfma(er[j], ei[j], vr[j], vi[j], xr, xi);
        vr[j] = live ? xr : 0.f;
        vi[j] = live ? xi : 0.f;
      }
      st4(u.v + ore, vr); st4(u.v + oim, vi);
    }
  }
}

// p <- p^2 over n4 float4 groups.  The field is a workspace piece, 256-byte aligned and padded to 256 bytes: the last
// group is whole also when B N is not a multiple of 4 (what it squares past the field is never read).
__global__ __launch_bounds__(256) void k_etd_square(float* __restrict__ p, long n4) {
  float4* __restrict__ q = reinterpret_cast<float4*>(p);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const float4 a = q[i];
    q[i] = make_float4(a.x * a.x, a.y * a.y, a.z * a.z, a.w * a.w);
  }
}

// rpde_etd1d_steps: Nv, a, the running sum, b / c and the product spectrum, and the field (the rfft / irfft calls need
// none)
struct EtdWork {
  float *nv, *a, *sum, *bc, *F, *P;
  EtdWork(Arena& ar, size_t spec, size_t phys)
      : nv(ar.take(spec)), a(ar.take(spec)), sum(ar.take(spec)), bc(ar.take(spec)), F(ar.take(spec)), P(ar.take(phys)) {}
};

// rpde_etd1d_steps (CX = false: seven real tables [kp]) and rpde_etd1d_steps_cx (six complex tables [re|im][kp] and
// the real g): the same checks, workspace and sixteen launches per step, the stage kernels of the table kind
template <bool CX>
static int etd1d_steps(float* U, const EtdTables& t, int B, int N, int nsteps, void* ws, size_t ws_bytes, void* stream) {
  const char* what = CX ? "etd1d_steps_cx" : "etd1d_steps";
  RPDE_CHECK_ARG(U && t.E && t.E2 && t.Q && t.f1 && t.f2 && t.f3 && t.g && ws, "%s: null pointer", what);
  if (CX) HS_CHECK_DIMS_1D("etd1d_steps_cx", B, N);
  else HS_CHECK_DIMS_1D("etd1d_steps", B, N);
  HS_CHECK_WS(what, ws);
  RPDE_CHECK_ARG(nsteps >= 0, "%s: nsteps %d < 0", what, nsteps);
  RPDE_CHECK_ARG(al16(U) && al16(t.E) && al16(t.E2) && al16(t.Q) && al16(t.f1) && al16(t.f2) && al16(t.f3) && al16(t.g),
                 "%s: state and tables must be 16-byte aligned", what);
  const HalfSpec geo = hs_geom(B, 1, N);
  const size_t phys = (size_t)B * N;
  RPDE_CARVE(what, EtdWork, w, ws, ws_bytes, hs_elems(geo), phys);
  const EtdBufs u{U, w.nv, w.a, w.sum, w.bc};
  float *F = w.F, *P = w.P;
  if (nsteps == 0) return RPDE_OK;
  hipStream_t st = as_stream(stream);
  // a wave per image of at most 64 groups (N <= 510), 256 threads otherwise
  const dim3 sb(hs_block(geo.kp / 4)), sg = hs_grid(geo.kp / 4, B, sb.x);
  const long n4 = ((long)phys + 3) / 4;
  // F = rfft(irfft(w)^2)
  auto product = [&](const float* w) -> int {
    RPDE_TRY(hs_irfft(geo, w, nullptr, P, st));
    hipLaunchKernelGGL(k_etd_square, dim3(hs_blocks(n4, 2048)), dim3(256), 0, st, P, n4);
    RPDE_LAUNCH_CHECK();
    return hs_rfft(geo, P, nullptr, F, st);
  };
  for (int j = 0; j < nsteps; ++j) {
    RPDE_TRY(product(u.v));
    hipLaunchKernelGGL(CX ? k_etd_stage_cx<0> : k_etd_stage<0>, sg, sb, 0, st, u, F, t, geo);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(product(u.a));
    hipLaunchKernelGGL(CX ? k_etd_stage_cx<1> : k_etd_stage<1>, sg, sb, 0, st, u, F, t, geo);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(product(u.bc));
    hipLaunchKernelGGL(CX ? k_etd_stage_cx<2> : k_etd_stage<2>, sg, sb, 0, st, u, F, t, geo);
    RPDE_LAUNCH_CHECK();
    RPDE_TRY(product(u.bc));
    hipLaunchKernelGGL(CX ? k_etd_stage_cx<3> : k_etd_stage<3>, sg, sb, 0, st, u, F, t, geo);
    RPDE_LAUNCH_CHECK();
  }
  return RPDE_OK;
}

}  // namespace rpde

using namespace rpde;

extern "C" {

size_t rpde_etd1d_spec_elems(int B, int N) { return hs_dims_ok(B, 1, N) ? hs_elems(hs_geom(B, 1, N)) : 0; }

size_t rpde_etd1d_ws_bytes(int B, int N) { return hs_dims_ok(B, 1, N) ? ws_measure<EtdWork>(hs_elems(hs_geom(B, 1, N)), (size_t)B * N) : 0; }

int rpde_etd1d_steps(float* U, const float* E, const float* E2, const float* Q, const float* f1, const float* f2,
                     const float* f3, const float* g, int B, int N, int nsteps, void* ws, size_t ws_bytes, void* stream) {
  return etd1d_steps<false>(U, EtdTables{E, E2, Q, f1, f2, f3, g}, B, N, nsteps, ws, ws_bytes, stream);
}

int rpde_etd1d_steps_cx(float* U, const float* E, const float* E2, const float* Q, const float* f1, const float* f2,
                        const float* f3, const float* g, int B, int N, int nsteps, void* ws, size_t ws_bytes,
                        void* stream) {
  return etd1d_steps<true>(U, EtdTables{E, E2, Q, f1, f2, f3, g}, B, N, nsteps, ws, ws_bytes, stream);
}

}  // extern "C"
