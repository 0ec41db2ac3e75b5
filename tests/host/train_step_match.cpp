// train_step_match.cpp -- walks dfa::match_step (csrc/train_step.h), the one decision whether a dfa_<model>_backward call is the
// backward of the forward_train its model's step record describes.  Pure host code: built by `make asan` with -fsanitize=address
// (host-only, nothing is launched) and run next to dfa_asan_harness by tests/test_host_api.py.
#include <stdio.h>

#include "train_step.h"

using namespace dfa;

int main() {
  TrainStep live;
  live.live = true;
  live.B = 2; live.T = 8; live.F = 20; live.prec = 1; live.x_dtype = 1; live.ragged = 0; live.synced = false;
  const StepCall same{2, 8, 20, 1, 0, false};
  TrainStep dead = live, ragged = live, hooked = live;
  dead.live = false;
  ragged.ragged = 1;
  hooked.synced = true;
  struct Row { const char* name; TrainStep s; StepCall c; bool f32_only; StepVerdict want; };
  const Row rows[] = {
      {"same batch", live, same, false, STEP_SAME},
      {"other B", live, {3, 8, 20, 1, 0, false}, false, STEP_OTHER_BATCH},
      {"other T", live, {2, 10, 20, 1, 0, false}, false, STEP_OTHER_BATCH},
      {"other F", live, {2, 8, 24, 1, 0, false}, false, STEP_OTHER_BATCH},
      {"ragged call, uniform forward", live, {2, 8, 20, 1, 1, false}, false, STEP_OTHER_BATCH},
      {"uniform call, ragged forward", ragged, same, false, STEP_OTHER_BATCH},
      {"ragged call, ragged forward", ragged, {2, 8, 20, 1, 1, false}, false, STEP_SAME},
      {"other x_dtype", live, {2, 8, 20, 0, 0, false}, false, STEP_OTHER_BATCH},
      {"other x_dtype, f32_only: the model's own refusal", live, {2, 8, 20, 0, 0, false}, true, STEP_SAME},
      {"f32_only still compares the shape", live, {2, 8, 24, 0, 0, false}, true, STEP_OTHER_BATCH},
      {"not live", dead, same, false, STEP_OTHER_BATCH},
      {"not live, f32_only", dead, same, true, STEP_OTHER_BATCH},
      {"a default record", TrainStep{}, {0, 0, 0, -1, 0, false}, false, STEP_OTHER_BATCH},
      {"hook armed since the forward", live, {2, 8, 20, 1, 0, true}, false, STEP_HOOK_CHANGED},
      {"hook cleared since the forward", hooked, same, false, STEP_HOOK_CHANGED},
      {"hook armed at both", hooked, {2, 8, 20, 1, 0, true}, false, STEP_SAME},
      {"another batch outranks a changed hook", live, {3, 8, 20, 1, 0, true}, false, STEP_OTHER_BATCH},
      {"not live outranks a changed hook", dead, {2, 8, 20, 1, 0, true}, false, STEP_OTHER_BATCH},
  };
  int failures = 0;
  for (const Row& r : rows) {
    const StepVerdict got = match_step(r.s, r.c, r.f32_only);
    if (got != r.want) {
      fprintf(stderr, "FAILED %s: verdict %d, want %d\n", r.name, (int)got, (int)r.want);
      ++failures;
    }
  }
  printf("train_step_match: %d row(s), %d failure(s)\n", (int)(sizeof(rows) / sizeof(rows[0])), failures);
  return failures ? 1 : 0;
}
