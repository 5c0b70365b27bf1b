// Which kernel arm does the dispatch plan (dalle-mtf_amd/csrc/gemm_plan.h) choose for a case of tests/test_gemm_exact_gpu.py?
// Host-only: reads one case per line from stdin and prints the arm's name, so tests/test_gemm_exact_ref.py can hold every case to the arm
// it is listed under, and the list to every arm of NtKernel and TnKernel, without a GPU.
//   NT M N K lda ldb k_per_split nsplit flags cus [option value]...
//   TN M I J cus [option value]...
#include <stdio.h>
#include <string.h>
#include <sstream>
#include <iostream>
#include <string>
#include "../../dalle-mtf_amd/csrc/gemm_plan.h"

static bool set_opt(GemmOptions& o, const std::string& k, int v) {
  const OptionSlot table[] = {{"nt4", &o.nt4}, {"nt8", &o.nt8}, {"nt8p", &o.nt8p}, {"ntr", &o.ntr}, {"skinny", &o.skinny}, {"res16", &o.res16},
                              {"tn8", &o.tn8}, {"tn_wide", &o.tn_wide}, {"tn_tail", &o.tn_tail}, {"reserve_cus", &o.reserve_cus}};
  return option_set(table, k.c_str(), v) == 0;
}

int main() {
  static const char* NT[] = {"SKINNY", "NTR", "NT8P", "NT8", "NT4", "NT2"};
  static const char* TN[] = {"TN", "TN8", "WIDE_SK", "TAIL"};
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind, k;
    int v;
    GemmOptions o;
    in >> kind;
    if (kind == "NT") {
      int M, N, K, lda, ldb, kps, nsplit, flags, cus;
      in >> M >> N >> K >> lda >> ldb >> kps >> nsplit >> flags >> cus;
      while (in >> k >> v)
        if (!set_opt(o, k, v)) return 2;
      // the compile-time facts of the epilogue (nt_traits in gemm.hip) for the flag sets of dmi_gemm_nt: the skinny kernel has
      // 0, BIAS, BIAS|RELU, BIAS|RESIDUAL; the register epilogue and the 256x128 kernel every bf16 output
      const bool f32 = (flags & 16) != 0;
      const NtTraits t = {flags == 0 || flags == 1 || flags == 3 || flags == 5, !f32, !f32, !f32, false};
      printf("%s\n", NT[(int)nt_plan(t, M, N, K, lda, ldb, kps, nsplit, o, cus).kernel]);
    } else if (kind == "TN") {
      int M, I, J, cus;
      in >> M >> I >> J >> cus;
      while (in >> k >> v)
        if (!set_opt(o, k, v)) return 2;
      printf("%s\n", TN[(int)tn_plan(M, I, J, o, cus).kernel]);
    } else {
      return 3;
    }
  }
  return 0;
}
