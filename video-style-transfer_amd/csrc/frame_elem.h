// Per-element arithmetic of the stylised-image tail, shared by the kernels that run its steps one at
// a time (tanh_image_kernel in loss_misc.hip, frames_to_tensor_* / tensor_to_frames_* in frames.hip)
// and the ones that fuse them (in_tanh_frames_kernel in norm.hip, conv_stem_u8_kernel in stem.hip), so
// the copies cannot drift.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// toTensor255 of a byte (RC/utilities.py:108-123): ToTensor (x / 255, IEEE division) then mul(255)
__device__ __forceinline__ float to255(uint32_t b) { return ((float)b / 255.0f) * 255.0f; }

// RT/network.py:93 on t = tanh(v): (t + 1) / 2 * 255
__device__ __forceinline__ float tanh_to_image(float th) { return ((th + 1.0f) / 2.0f) * 255.0f; }

// Inference.__iter__ (RC/utilities.py:213-219, RT/utilities.py:328-330): clamp(0, 255) ...
__device__ __forceinline__ float clamp255(float v) { return v < 0.f ? 0.f : (v > 255.f ? 255.f : v); }

// ... then numpy float32 -> uint8 (C truncation) of the clamped value
__device__ __forceinline__ uint32_t to_u8(float v) { return (uint32_t)(int)v; }
