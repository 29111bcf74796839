/* Stand-in for the CUDA toolkit's cuda_runtime.h, for compiling the reference's header-only classes (R/*.h) as host C++
 * (oracle/ref_world.cpp).  The headers use nothing of the runtime but the function qualifiers, which mean nothing on a host. */
#pragma once
#define __device__
#define __host__
#define __global__
