// The CPU wave emulator's harness (emu_main.cpp) plus the entries tests/test_proximity_cpu.py needs: the wave body of the closest-point query
// (csrc/agx_proximity.h prox_wave) under run_wave, one emulated wavefront per wave of the launch, and the body of the frames kernel
// (csrc/agx_kernels.hip agx_frames_kernel) that feeds it.  Built by that test into tests/emu/libagx_emu_proximity_<kind>.so.  Test-only.
#include "emu_main.cpp"
#include "agx_proximity.h"

// frames[ncoll][12] of one environment, as the frames kernel writes them
extern "C" int agx_emu_collider_frames(const uint32_t* blob, const float* state, float* frames) {
  static float lds[agx::LDS_WORDS];
  const int sw = ((const int*)blob)[AGX_H_STATE_WORDS];
  return run_wave(lds, agx::LDS_WORDS, [&](int lane) {
    agx::Ctx c; agx::ctx_init(c, blob, lds, lane);
    agx::load_env(c, state, sw);
    agx::kinematics(c);
    for (int col = lane; col < c.ncoll; col += 64) {
      m3 R; v3 p; agx::body_xf(c, CLI(c, col, AGX_C_BODY), R, p);
      st3(frames + 12 * col, p); stm3(frames + 12 * col + 3, R);
    }
  });
}
// agx_proximity of the environments [env0, env0 + count): states [n][sw], frames [n][ncoll][12], pairs [npairs][4], flags [ncoll] (csrc/agx_proximity.h);
// group as agx_proximity_set chooses it.  < 0 on divergent control flow.
extern "C" int agx_emu_proximity(const uint32_t* blob, const float* states, int sw, const float* frames, const int* pairs4, const int* cflags, int npairs, int nqueries,
                                 int env0, int count, float max_distance, float* records, float* nearest) {
  static float lds[64];
  agx_prox_args A;
  memset(&A, 0, sizeof A);
  A.blob = blob; A.state = states; A.sw = sw; A.frames = frames; A.pairs = pairs4; A.cflags = cflags; A.npairs = npairs; A.nqueries = nqueries;
  int G = 1; while (G < AGX_WAVE && (G < npairs || G < nqueries)) G <<= 1;
  A.group = G; A.env0 = env0; A.count = count; A.max_distance = max_distance; A.records = records; A.nearest = nearest;
  const int per_wave = AGX_WAVE / G, waves = (count + per_wave - 1) / per_wave;
  for (int w = 0; w < waves; w++)
    if (run_wave(lds, 64, [&](int lane) { agxprox::prox_wave(A, w, lane); })) return -1;
  return 0;
}
