// The CPU wave emulator's harness (emu_main.cpp) plus the entries tests/test_emu_solve_pair.py needs: one wavefront that solves TWO environments as a
// workgroup of the paired solve kernel does (csrc/agx_env.h env_solve_pair, csrc/agx_pgs_lvw.h pgs_lvw_pair).  Built by that test into
// tests/emu/libagx_emu_pair_<kind>.so.  Test-only.
#include "emu_main.cpp"

extern "C" int agx_emu_pair_scr_words() { return agx::SCR_WORDS; }
extern "C" int agx_emu_pair_meta(int* out4) { out4[0] = agx::SCR_O_META + agx::META_NROWS; out4[1] = agx::SCR_O_META + agx::META_NCON; out4[2] = agx::LVW_MAX_STEPS; out4[3] = AGX_SOLVE_PAIR; return 0; }
// the build pass of one environment into the given scratch record
extern "C" int agx_emu_pair_build(const uint32_t* blob, float* state, const float* action, float* scratch) {
  static float lds[agx::LDS_WORDS];
  return run_wave(lds, agx::LDS_WORDS, [&](int lane) { agx::env_build<true>(blob, state, action, scratch, nullptr, lds, lane); });
}
// The solve pass of the two environments whose state records (sw words each) and scratch records follow each other, as a workgroup of the solve kernel
// treats them (csrc/agx_kernels.hip): present bit e = environment e takes part.  paired = 0: one env_solve after the other, each on its own LDS, as the
// kernel of an unpaired build.  Returns 1 when the paired sweep ran, 0 when the environments went through env_solve, < 0 on divergent control flow.
extern "C" int agx_emu_pair_solve(const uint32_t* blob, float* states, int sw, float* scratch, int phase, int paired, int present) {
  static float lds[2 * EMU_SOLVE_WORDS];
  const bool has0 = present & 1, has1 = present & 2;
  int rc = 0, took = 0;
#if AGX_SOLVE_PAIR
  if (paired) {
    rc = run_wave(lds, 2 * EMU_SOLVE_WORDS, [&](int lane) {
      if (has0 && has1 && agx::env_solve_pair(blob, states, scratch, lds, lane, phase, EMU_SOLVE_WORDS)) { if (lane == 0) took = 1; return; }
      for (int e = 0; e < 2; e++) {
        if (e ? has1 : has0) agx::env_solve(blob, states + (size_t)e * sw, scratch + (size_t)e * agx::SCR_WORDS, nullptr, lds, lane, phase, EMU_SOLVE_WORDS);
        wave_sync();
      }
    });
    return rc ? -1 : took;
  }
#endif
  for (int e = 0; e < 2 && !rc; e++)
    if (e ? has1 : has0) rc = run_wave(lds, EMU_SOLVE_WORDS, [&](int lane) { agx::env_solve(blob, states + (size_t)e * sw, scratch + (size_t)e * agx::SCR_WORDS, nullptr, lds, lane, phase, EMU_SOLVE_WORDS); });
  return rc ? -1 : 0;
}
// the list schedules of a scratch record's rows `ng` rows wide (csrc/agx_pgs_lvw.h lvw_schedule): out[0..1] = steps of the non-contact + normal part and of
// the friction part (-1: does not fit LVW_MAX_STEPS), out[2..4] = rows, non-contact rows, contacts; ssA64 / ssF64 (may be null): the rows of every step
extern "C" int agx_emu_pair_schedule(float* scratch, int ng, int* out, uint32_t* ssA64, uint32_t* ssF64) {
  static float lds[64];
  const int* m = (const int*)(scratch + agx::SCR_O_META);
  const int R = m[agx::META_NROWS], nnc = m[agx::META_NNC], nc = m[agx::META_NCON];
  out[2] = R; out[3] = nnc; out[4] = nc;
  return run_wave(lds, 64, [&](int lane) {
    agx::Ctx c; c.H = scratch + agx::SCR_O_HDR; c.lane = lane;
    uint32_t a, f;
    const int nsA = agx::lvw_schedule(c, lane, 0, nnc + nc, a, ng), nsF = agx::lvw_schedule(c, lane, nnc + nc, nc, f, ng);
    if (ssA64) ssA64[lane] = a;
    if (ssF64) ssF64[lane] = f;
    if (lane == 0) { out[0] = nsA; out[1] = nsF; }
  });
}
