// csrc/agx_ik.h compiled with g++ under the emulator's shim (tests/emu/agx_wave.h: AGX_DEV): the device's end-effector math, one
// (environment, arm) per call.  The iteration loop's wave-wide ballot is the lane's own flag here.  Built by tests/test_ee_cpu.py into
// tests/emu/libagx_ik_host.so.  Test-only.
#include "agx_wave.h"
#include "agx_ik.h"

extern "C" void ik_host_pose(const uint32_t* blob, const float* state, int arm, float* pose7) { agxik::lane_pose(blob, state, arm, pose7); }

extern "C" void ik_host_ik(const uint32_t* blob, const float* state, int arm, const float* target, int frame, int iters, float damping, float gain,
                           float* q_out7, float* err2, float* action_row) {
  agxik::lane_ik(blob, state, arm, target, frame, iters, damping, gain, q_out7, err2, action_row, true, [](bool stopped) { return stopped; });
}
