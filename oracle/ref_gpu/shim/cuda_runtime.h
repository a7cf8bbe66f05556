/* Redirect for building the reference's CUDA sources with hipcc: the nine runtime names they use. */
#pragma once
#include <hip/hip_runtime.h>
#define cudaSuccess hipSuccess
#define cudaError_t hipError_t
#define cudaDeviceSynchronize hipDeviceSynchronize
#define cudaGetErrorString hipGetErrorString
#define cudaMemcpy hipMemcpy
#define cudaMemcpyDeviceToHost hipMemcpyDeviceToHost
#define cudaMemset hipMemset
#define cudaMalloc hipMalloc
#define cudaFree hipFree
