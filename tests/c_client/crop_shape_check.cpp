// Host check of crop_shape (tepose_amd/csrc/shapes.h): the launch of crop_frames_u8_kernel / crop_boxes_u8_kernel -- one thread per crop pixel in
// blocks of 256, one grid row per crop up to 65535 -- covers every pixel of every crop at the sizes the entry points admit, and stays inside the
// limits of a grid.  Plain C++: the header includes nothing from HIP.
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
  const int sides[] = {1, 2, 8, 15, 16, 17, 224, 255, 256, 257, 1000, 32767, kCropMaxSide};
  const int counts[] = {1, 2, 6, 8, 64, 4095, kSessionMaxSlots, 65534, 65535, 65536, 100000};
  for (int S : sides)
    for (int n : counts) {
      const Launch l = crop_shape(S, n);
      const long px = (long)S * S;
      CHECK(l.threads == 256u && l.gz == 1u && l.kernel == 0);
      CHECK((long)l.gx * l.threads >= px);                  // every pixel has a thread
      CHECK(((long)l.gx - 1) * l.threads < px);             // and no block is idle
      CHECK(l.gx >= 1u && l.gx <= (1u << 22));              // far below the 2^31 - 1 blocks of grid x
      CHECK(l.gy >= 1u && l.gy <= 65535u && l.gy == (unsigned)(n < 65535 ? n : 65535));      // grid y's limit; rows stride above it
      CHECK((long)(l.gx - 1) * l.threads + (l.threads - 1) < (1L << 31));                    // the pixel index fits an int
      ++combos;
    }
  // what DESIGN.md section 18 states: a session tick of S = 8 crops of 224 x 224 is 196 x 8 blocks
  const Launch t = crop_shape(224, 8);
  CHECK(t.gx == 196u && t.gy == 8u);
  CHECK(kSessionMaxSlots <= 65535);                         // tepose_crop_boxes_u8's n limit: one grid row per crop, never a stride
  if (fails) return 1;
  printf("ok %d\n", combos);
  return 0;
}
