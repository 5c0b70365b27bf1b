// The compiler's layout of the two structs of include/dalle_hip.h, for tests/test_abi_header.py to compare with the ctypes
// Structures that dalle_hip builds from the same header: one line "<struct> sizeof <bytes>", then "<struct>.<field> <offset>" per
// field.  Includes the public header and nothing else of the project, so it also shows that the header compiles on its own.
#include <cstddef>
#include <cstdio>

#include "../../include/dalle_hip.h"

#define SIZE(T) std::printf(#T " sizeof %zu\n", sizeof(T))
#define FIELD(T, f) std::printf(#T "." #f " %zu\n", offsetof(T, f))

int main() {
  SIZE(dmi_reduce_item);
  FIELD(dmi_reduce_item, slabs);
  FIELD(dmi_reduce_item, out);
  FIELD(dmi_reduce_item, nsplit);
  FIELD(dmi_reduce_item, n4);
  SIZE(dmi_tn_problem);
  FIELD(dmi_tn_problem, X);
  FIELD(dmi_tn_problem, ldx);
  FIELD(dmi_tn_problem, dY);
  FIELD(dmi_tn_problem, ldy);
  FIELD(dmi_tn_problem, dW);
  FIELD(dmi_tn_problem, dbias);
  FIELD(dmi_tn_problem, bias_weights);
  FIELD(dmi_tn_problem, I);
  FIELD(dmi_tn_problem, J);
  FIELD(dmi_tn_problem, workspace);
  std::printf("abi_layout_check: ok\n");
  return 0;
}
