// ref_launch.hip -- launcher around the reference's own three index kernels.  TEST INFRASTRUCTURE ONLY.
//
// oracle/ref_kernels.py cuts the kernel text out of a reference checkout (misc/ops.py) into oracle/_ref/*.inc and compiles
// this file around it, once with -ffp-contract=off and once with -ffp-contract=fast.  Nothing of the reference is in this
// file: it holds the launches that the reference writes as jt.code host snippets (misc/ops.py:236-251, :332-337, :562-638),
// restated for HIP.  Every entry point takes device pointers and a stream, launches, and returns hipGetLastError().
#include <hip/hip_runtime.h>

#include "fps.inc"
#include "ball_query.inc"
#include "knn.inc"

// misc/ops.py:241-249: grid B, block_size threads, 2*block_size ints of dynamic LDS.  `temp` [B,N] floats is the caller's
// (the reference allocates it as managed memory per call).  The reduction tree of the kernel starts at 512 -> 256, so
// block_size must be a power of two in [1, 512].
extern "C" int ref_fps(const float* xyz, float* temp, int* idx, int B, int N, int m, int block_size, hipStream_t stream) {
    if (!xyz || !temp || !idx || B < 1 || N < 1 || m < 1 || m > N) return (int)hipErrorInvalidValue;
    if (block_size < 1 || block_size > 512 || (block_size & (block_size - 1))) return (int)hipErrorInvalidValue;
    (void)hipGetLastError();
    furthest_point_sampling_kernel<<<dim3(B), dim3(block_size), 2 * block_size * sizeof(int), stream>>>(B, N, m, block_size, xyz, temp, idx);
    return (int)hipGetLastError();
}

// misc/ops.py:334-337: grid B, block_size threads; b, n (cloud), m (queries), radius, nsample, new_xyz, xyz, idx, cnt.
extern "C" int ref_ball_query(const float* new_xyz, const float* xyz, int* idx, int* cnt, int B, int N, int m, float radius,
                              int nsample, int block_size, hipStream_t stream) {
    if (!new_xyz || !xyz || !idx || !cnt || B < 1 || N < 1 || m < 1 || nsample < 1) return (int)hipErrorInvalidValue;
    if (block_size < 1 || block_size > 1024) return (int)hipErrorInvalidValue;
    (void)hipGetLastError();
    query_ball_point_kernel<<<dim3(B), dim3(block_size), 0, stream>>>(B, N, m, radius, nsample, new_xyz, xyz, idx, cnt);
    return (int)hipGetLastError();
}

// knn_cuda_global, misc/ops.py:588-619: pitches are the point counts; distances on a ceil(Nq/16) x ceil(Nr/16) x B grid of
// 16x16 blocks into dist [B,Nr,Nq]; the insertion sort on a ceil(Nq/256) x 1 x B grid of 256 threads into idx [B,k,Nq].
extern "C" int ref_knn(const float* ref, const float* query, float* dist, int* idx, int B, int C, int Nr, int Nq, int k,
                       hipStream_t stream) {
    if (!ref || !query || !dist || !idx || B < 1 || C < 1 || Nr < 1 || Nq < 1 || k < 1 || k > Nr) return (int)hipErrorInvalidValue;
    const int BLOCK_DIM = 16;
    dim3 block0(BLOCK_DIM, BLOCK_DIM, 1);
    dim3 grid0((Nq + BLOCK_DIM - 1) / BLOCK_DIM, (Nr + BLOCK_DIM - 1) / BLOCK_DIM, B);
    if (grid0.y > 65535 || grid0.z > 65535) return (int)hipErrorInvalidValue;
    (void)hipGetLastError();
    compute_distances<<<grid0, block0, 0, stream>>>(const_cast<float*>(ref), Nr, Nr, const_cast<float*>(query), Nq, Nq, C, dist);
    int rc = (int)hipGetLastError();
    if (rc) return rc;
    dim3 block1(256, 1, 1);
    dim3 grid1((Nq + 255) / 256, 1, B);
    modified_insertion_sort<<<grid1, block1, 0, stream>>>(dist, Nr, idx, Nq, Nq, Nr, k);
    return (int)hipGetLastError();
}
