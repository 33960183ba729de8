// The LSTM cell's gate arithmetic (torch.nn.LSTMCell, gate order i | f | g | o), written once for the rollout's launch (bg_actor_mlp.hip:
// bg_actor_sample_lstm) and the update's recurrence (bg_lstm.hip): the state an actor carries through a rollout and the state the update recomputes
// come out of the same expressions.  The x-side and the h-side pre-activations simply add, so a gate takes their SUM, p = gi + gh:
//     i = sigmoid(p_i), f = sigmoid(p_f), g = tanh(p_g), o = sigmoid(p_o), c' = f c + i g, h' = o tanh(c')
#pragma once
#include <hip/hip_runtime.h>

namespace bg {

struct LstmGates { float i, f, g, o, c, tanh_c, h; };  // c, h: the new states; tanh_c = tanh(c'), which the backward pass reads

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ LstmGates lstm_gates(float p_i, float p_f, float p_g, float p_o, float c) {
    LstmGates s;
    s.i = lstm_sigmoid(p_i);
    s.f = lstm_sigmoid(p_f);
    s.g = tanhf(p_g);
    s.o = lstm_sigmoid(p_o);
    s.c = s.f * c + s.i * s.g;
    s.tanh_c = tanhf(s.c);
    s.h = s.o * s.tanh_c;
    return s;
}

}  // namespace bg
