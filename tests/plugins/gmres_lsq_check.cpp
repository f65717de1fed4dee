// gmres_lsq_check.cpp -- drives fluca_amd/csrc/fl_gmres_lsq.h with the host compiler alone (tests/test_gmres_lsq_host.py).
// stdin: k, beta, then the (k+1) x k upper-Hessenberg matrix row by row (any form strtod reads, hexadecimal included).
// stdout: "E <value>" after every column -- the residual estimate GmresLsq::push returns -- then "Y <value>" for y[0 .. k); all with %a.
#include <cstdio>
#include <vector>

#include "../../fluca_amd/csrc/fl_gmres_lsq.h"

int main()
{
  int    k = 0;
  double beta = 0.;
  if (std::scanf("%d %lf", &k, &beta) != 2 || k < 1 || k > 1000) return 2;
  std::vector<double> H((size_t)(k + 1) * k), col((size_t)k + 1), y((size_t)k);
  for (double &v : H)
    if (std::scanf("%lf", &v) != 1) return 2;
  fl::GmresLsq lsq(k);
  lsq.reset(beta);
  for (int j = 0; j < k; ++j) {
    for (int i = 0; i <= j + 1; ++i) col[(size_t)i] = H[(size_t)i * k + j];
    std::printf("E %a\n", lsq.push(j, col.data()));
  }
  lsq.solve(k, y.data());
  for (int i = 0; i < k; ++i) std::printf("Y %a\n", y[(size_t)i]);
  return 0;
}
