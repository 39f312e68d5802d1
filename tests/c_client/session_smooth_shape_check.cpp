// Host check of session_smooth_shape (tepose_amd/csrc/shapes.h): the launch of session_smooth_kernel -- one thread per (slot, theta column) in blocks
// of 128 -- gives every one of the S * 85 columns a thread at each slot count tepose_session_smooth admits, leaves no block idle, and keeps the
// flat index and the offsets formed from it inside an int.  Plain C++: the header includes nothing from HIP.
#include <stdio.h>

#include "shapes.h"

using namespace tepose;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      ++fails;                                                    \
      printf("FAIL line %d: %s\n", __LINE__, #c);                 \
    }                                                             \
  } while (0)

int main() {
  int combos = 0;
  const int slots[] = {1, 2, 3, 8, 63, 64, 65, 127, 128, 1000, 4095, kSessionMaxSlots};
  for (int S : slots) {
    const Launch l = session_smooth_shape(S);
    const long cols = (long)S * kTheta;
    CHECK(l.threads == 128u && l.gy == 1u && l.gz == 1u && l.kernel == 0);
    CHECK((long)l.gx * l.threads >= cols);                  // every (slot, column) has a thread
    CHECK(((long)l.gx - 1) * l.threads < cols);             // and no block is idle
    CHECK(l.gx >= 1u && (long)l.gx * l.threads < (1L << 31));      // the flat index fits an int
    const Launch c = session_commit_shape(S);               // the same walk as the commit's: one rule for both (slot, theta column) kernels
    CHECK(c.gx == l.gx && c.threads == l.threads);
    ++combos;
  }
  // the largest offsets the kernel forms as int: s * 72 and s * 10 of the contiguous outputs
  CHECK((long)kSessionMaxSlots * kTheta < (1L << 31) && (long)kSessionMaxSlots * 144 < (1L << 31));
  // what DESIGN.md section 17 states: S = 8 is 680 threads = 6 blocks; one slot is one block
  CHECK(session_smooth_shape(8).gx == 6u && session_smooth_shape(1).gx == 1u);
  CHECK(kTheta == 85);
  if (fails) return 1;
  printf("ok %d\n", combos);
  return 0;
}
