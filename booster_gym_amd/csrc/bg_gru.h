// The GRU cell's gate arithmetic (torch.nn.GRUCell, gate order r | z | n), written once for the rollout's launch (bg_actor_mlp.hip: bg_actor_sample_gru,
// bg_distill_act_gru) and the update's recurrence (bg_gru.hip): the state a student carries through a rollout and the state the update recomputes
// come out of the same expressions.
//     r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h
#pragma once
#include <hip/hip_runtime.h>

namespace bg {

struct GruGates { float r, z, n, h; };

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ GruGates gru_gates(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n, float h) {
    GruGates g;
    g.r = gru_sigmoid(gi_r + gh_r);
    g.z = gru_sigmoid(gi_z + gh_z);
    g.n = tanhf(gi_n + g.r * gh_n);
    g.h = (1.0f - g.z) * g.n + g.z * h;
    return g;
}

}  // namespace bg
