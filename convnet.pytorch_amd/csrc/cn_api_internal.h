// cn_api_internal.h -- internal declarations shared by the translation units of libconvnet_hip.so.
#pragma once
#include "cn_common.h"
#include <string.h>
// the public C ABI: every definition is compiled against its declaration
#include "../../include/convnet_hip.h"

// ---- helpers defined in one source and called from another (each declared here, once) ----
// wgrad.hip: fixed-order reduction of the split partial products (also behind stem.hip's and gconv.hip's weight gradients)
int wg_launch_reduce(hipStream_t stream, const float* part, float* dw, int nsplit, int Co, int ntaps, int Ci, int Creal,
                     float beta, float scale);
// dense.hip: small-M dense product behind igemm.hip's 1x1-image convolutions (returns 1: not a shape it takes)
int cn_dense_smallm(const void* A, const void* B, void* C, const float* bias, int M, int N, int Kd, int dtype, int out_f32,
                    int relu, hipStream_t stream);
// plan.hip: what runtime.hip's hand-offs and comm.hip's collectives log while a launch plan is being recorded
void cn_plan_rec_fork(void* from, void* to);
int cn_plan_rec_wait_mark(int handle, void* to);
void cn_plan_rec_comm(int kind, void* comm, void* buf, long long count, int dtype, void* s0, void* s1, int n_after);
// comm.hip: the communicator entry points that really issue (a plan's replay calls them)
int cn_comm_allreduce_bucket_issue(void* handle, float* buf, long long count, void* after_a, void* after_b, int n_after);
int cn_comm_join_issue(void* handle, void* stream);
int cn_comm_allreduce_issue(void* handle, void* buf, long long count, int dtype, void* stream);
