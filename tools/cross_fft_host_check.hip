// CPU emulation of the K25 wave program (csrc/cross_spectrum.hip): runs the
// per-lane code of weatherbench2_amd/csrc/fft_core.hpp lane by lane on a truth
// row and a forecast row (every read phase of a pass before its write phase,
// the order the DS queue of one wave enforces), recombines both with
// recombine_pair_complex, forms the four terms as the kernel does (float32
// products, widened and scaled by s_k) and compares them with a direct O(N^2)
// DFT in double.
//
//   hipcc --cuda-host-only -O2 -std=c++17 -I weatherbench2_amd/csrc \
//       tools/cross_fft_host_check.hip -o /tmp/cross_check && /tmp/cross_check
//
// Prints one line per instantiated size:
//   "N <n_lon> pf <e> pt <e> co <e> qu <e>"
// e = max_k |got - ref| over sum_k |ref| for the powers and over
// sqrt(sum pf * sum pt) for the cospectrum and the quadrature.
#include "fft_core.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace wb2::fftcore;

template <typename P, int R, bool FIRST>
void run_pass(std::vector<cf>& z, const std::vector<cf>& twz, const float* x) {
  static cf v[kLanes][P::ROUNDS][R];
  for (int lane = 0; lane < kLanes; ++lane) {
    if constexpr (FIRST) {
      P::load([&](int i) { return cf{x[2 * i], x[2 * i + 1]}; }, lane, v[lane]);
    } else {
      cf tw[P::ROUNDS][P::NTW];
      P::load_twiddles(twz.data(), lane, tw);
      P::load([&](int i) { return z[i]; }, lane, v[lane]);
      P::twiddle(v[lane], tw);
    }
    P::butterflies(v[lane]);
  }
  for (int lane = 0; lane < kLanes; ++lane) P::store(z.data(), lane, v[lane]);
}

template <int N2>
std::vector<cf> transform(const std::vector<cf>& twz, const float* x) {
  using PL = Plan<N2>;
  using P0 = Pass<N2, PL::R0, 1, 1, 0, PL::PAD0>;
  using P1 = Pass<N2, PL::R1, PL::R0, PL::R0, PL::PAD0, PL::PAD1>;
  using P2 = Pass<N2, PL::R2, PL::R0 * PL::R1, PL::R0 * PL::R1, PL::PAD1, 0>;
  std::vector<cf> z(slab_slots<N2>(), cf{0.0f, 0.0f});
  run_pass<P0, PL::R0, true>(z, twz, x);
  run_pass<P1, PL::R1, false>(z, twz, x);
  if constexpr (PL::R2 > 1) run_pass<P2, PL::R2, false>(z, twz, x);
  return z;
}

static void dft(const std::vector<float>& x, std::vector<double>& re,
                std::vector<double>& im) {
  const int n = (int)x.size();
  for (int k = 0; k <= n / 2; ++k) {
    double a = 0.0, b = 0.0;
    for (int j = 0; j < n; ++j) {
      const double w = 2.0 * kPi * (double)((long long)j * k % n) / n;
      a += x[j] * std::cos(w);
      b -= x[j] * std::sin(w);
    }
    re[k] = a / n;
    im[k] = b / n;
  }
}

struct Errors {
  double e[4];
};

template <int N2>
Errors check(unsigned seed) {
  constexpr int N = 2 * N2, NH = N2 / 2 + 1, NB = N2 + 1;
  std::vector<cf> twz(N2), twq(NH);
  for (int j = 0; j < N2; ++j) {
    const double a = 2.0 * kPi * j / N2;
    table_entry_z(j, N2, std::cos(a), std::sin(a), twz[j]);
  }
  for (int k = 0; k < NH; ++k) {
    const double a = kPi * k / N2;
    table_entry_q(N2, std::cos(a), std::sin(a), twq[k]);
  }
  // N(0, 1)-like rows with a mean of 3, the forecast correlated with the truth
  std::vector<float> t(N), f(N);
  srand(seed);
  auto unit = [] { return rand() / (double)RAND_MAX - 0.5; };
  for (int i = 0; i < N; ++i) {
    const double a = 3.46 * unit(), b = 3.46 * unit();
    t[i] = (float)(a + 3.0);
    f[i] = (float)(0.8 * a + 0.6 * b + 3.0);
  }
  const std::vector<cf> zt = transform<N2>(twz, t.data());
  const std::vector<cf> zf = transform<N2>(twz, f.data());
  std::vector<double> got[4], ref[4];
  for (int s = 0; s < 4; ++s) {
    got[s].assign(NB, 0.0);
    ref[s].assign(NB, 0.0);
  }
  const float half_inv_n = 0.5f / (float)N;
  constexpr int NIT = (NH + kLanes - 1) / kLanes;
  for (int lane = 0; lane < kLanes; ++lane)
    for (int i = 0; i < NIT; ++i) {
      const int k = lane + i * kLanes;
      if (k >= NH) continue;
      const int km = k == 0 ? 0 : N2 - k;
      cf t1, t2, f1, f2;
      recombine_pair_complex(zt[k], zt[km], twq[k], half_inv_n, t1, t2);
      recombine_pair_complex(zf[k], zf[km], twq[k], half_inv_n, f1, f2);
      const double s1 = k == 0 ? 1.0 : 2.0;
      got[0][k] = (double)(f1.x * f1.x + f1.y * f1.y) * s1;
      got[1][k] = (double)(t1.x * t1.x + t1.y * t1.y) * s1;
      got[2][k] = (double)(f1.x * t1.x + f1.y * t1.y) * s1;
      got[3][k] = (double)(f1.y * t1.x - f1.x * t1.y) * s1;
      if (2 * k != N2) {
        got[0][N2 - k] = (double)(f2.x * f2.x + f2.y * f2.y) * 2.0;
        got[1][N2 - k] = (double)(t2.x * t2.x + t2.y * t2.y) * 2.0;
        got[2][N2 - k] = (double)(f2.x * t2.x + f2.y * t2.y) * 2.0;
        got[3][N2 - k] = (double)(f2.y * t2.x - f2.x * t2.y) * 2.0;
      }
    }
  std::vector<double> tr(NB), ti(NB), fr(NB), fi(NB);
  dft(t, tr, ti);
  dft(f, fr, fi);
  double tot_f = 0.0, tot_t = 0.0;
  for (int k = 0; k < NB; ++k) {
    const double s = k == 0 ? 1.0 : 2.0;
    ref[0][k] = (fr[k] * fr[k] + fi[k] * fi[k]) * s;
    ref[1][k] = (tr[k] * tr[k] + ti[k] * ti[k]) * s;
    ref[2][k] = (fr[k] * tr[k] + fi[k] * ti[k]) * s;
    ref[3][k] = (fi[k] * tr[k] - fr[k] * ti[k]) * s;
    tot_f += ref[0][k];
    tot_t += ref[1][k];
  }
  const double scale[4] = {tot_f, tot_t, std::sqrt(tot_f * tot_t),
                           std::sqrt(tot_f * tot_t)};
  Errors out{};
  for (int s = 0; s < 4; ++s) {
    double err = 0.0;
    for (int k = 0; k < NB; ++k)
      err = std::fmax(err, std::fabs(got[s][k] - ref[s][k]));
    out.e[s] = err / scale[s];
  }
  return out;
}

int main() {
  double worst[4] = {0.0, 0.0, 0.0, 0.0};
#define WB2_CHECK(N2)                                                      \
  {                                                                        \
    const Errors e = check<N2>(4321u + N2);                                \
    std::printf("N %d pf %.3e pt %.3e co %.3e qu %.3e\n", 2 * N2, e.e[0],  \
                e.e[1], e.e[2], e.e[3]);                                   \
    for (int s = 0; s < 4; ++s) worst[s] = std::fmax(worst[s], e.e[s]);    \
  }
  WB2_FFT_PLAN_SIZES(WB2_CHECK)
  std::printf("worst pf %.3e pt %.3e co %.3e qu %.3e\n", worst[0], worst[1],
              worst[2], worst[3]);
  return 0;
}
