/* The tile scheduler's settings of one call (free positions per segment: mode bit 4 plans wide tiles) must not outlive the
 * call, whichever way it ends.  Plans a circuit in mode 1|16 that fails classification mid-way, then a good circuit in mode 1,
 * and compares that plan's step count with the one a fresh process gets.  Host code only, no device.
 *   test_plan_settings          the check (starts itself once more with "fresh")
 *   test_plan_settings fresh    prints the good circuit's step count */
#define _POSIX_C_SOURCE 200809L /* popen */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qip_hip.h"

enum { N = 14, GOOD = 7 };
/* amplitude-index positions above the rows of a Complex<f64> tile at n = 14 (rows: 0..4 and 11): a Hadamard on each of seven is
 * one segment with seven free positions and two with five */
static const uint32_t kPos[GOOD] = {5, 6, 7, 8, 9, 10, 12};
static const qip_c64 kH[4] = {{0.70710678118654757, 0}, {0.70710678118654757, 0}, {0.70710678118654757, 0}, {-0.70710678118654757, 0}};

static int plan(int mode, uint64_t bad_index_at, uint64_t* n_steps) {
  uint64_t idx[GOOD];
  qip_op ops[GOOD];
  int64_t step_of[GOOD];
  memset(ops, 0, sizeof ops);
  for (uint64_t i = 0; i < GOOD; ++i) {
    idx[i] = i == bad_index_at ? (uint64_t)N + 3 : (uint64_t)(N - 1) - kPos[i];
    ops[i].kind = QIP_OP_MATRIX;
    ops[i].n_indices = 1;
    ops[i].indices = &idx[i];
    ops[i].dense = kH;
  }
  return qip_hip_plan_tiles(QIP_C64, N, ops, GOOD, mode, step_of, n_steps);
}

int main(int argc, char** argv) {
  uint64_t steps = 0;
  if (argc > 1 && !strcmp(argv[1], "fresh")) {
    if (plan(1, GOOD, &steps) != QIP_OK) return 2;
    printf("%llu\n", (unsigned long long)steps);
    return 0;
  }
  uint64_t wide = 0;
  if (plan(1 | 16, GOOD, &wide) != QIP_OK) return fprintf(stderr, "wide plan: %s\n", qip_hip_last_error()), 1;
  if (plan(1 | 16, GOOD - 2, &steps) == QIP_OK) return fprintf(stderr, "the op with a bad index was accepted\n"), 1;
  if (plan(1, GOOD, &steps) != QIP_OK) return fprintf(stderr, "plan: %s\n", qip_hip_last_error()), 1;
  char cmd[4096];
  unsigned long long fresh = 0;
  snprintf(cmd, sizeof cmd, "'%s' fresh", argv[0]);
  FILE* p = popen(cmd, "r");
  if (!p || fscanf(p, "%llu", &fresh) != 1 || pclose(p) != 0) return fprintf(stderr, "no step count from a fresh process\n"), 1;
  printf("steps: wide %llu, after the failed wide call %llu, fresh process %llu\n", (unsigned long long)wide, (unsigned long long)steps, fresh);
  if (wide >= fresh) return fprintf(stderr, "the circuit does not tell wide plans from narrow ones\n"), 1;
  if (steps != fresh) return fprintf(stderr, "FAILED: a failed call left its settings behind\n"), 1;
  printf("PASSED\n");
  return 0;
}
