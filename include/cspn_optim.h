/*
 * cspn_optim.h — C ABI of the reference's optimiser step in libcspn_hip.so (paths relative to the reference repo):
 *   main.py:72-74                              torch.optim.SGD(lr, momentum 0.9, weight_decay 1e-4)
 *   libs/trainers/single_gpu_trainer.py        train_iter: self.optimizer.step()
 * as ONE multi-tensor kernel: a launch updates up to CSPN_SGD_TENSORS_PER_LAUNCH tensors of one parameter group, without atomics,
 * without LDS, without a host synchronisation and capturable in a graph.
 *
 * A header of its own with a version of its own: CSPN_ABI_VERSION (cspn_hip.h) does not move.  The conventions are those of
 * cspn_losses.h: 1 on success, 0 on failure + cspn_last_error(); the caller owns every buffer, selects the device, and the library
 * enqueues on the given stream without synchronising; the host arrays are only read during the call.  dtype: CSPN_F32 only.
 *
 * Arithmetic: that of torch.optim.SGD(foreach=False, fused=False), per element, in fp32.  Every scalar is rounded to fp32 first;
 * 1 - dampening is formed in double and then rounded (as Python forms it).
 *     g   = maximize ? -grad : grad
 *     g   = fma(wd, p, g)                                   if weight_decay != 0
 *     buf = g                                               on a tensor's first step (a copy: -0.0 stays -0.0; buf is not read)
 *     buf = fma(1 - dampening, g, fl(momentum * buf))       otherwise: the product is rounded ON ITS OWN
 *     d   = nesterov ? fma(momentum, buf, g) : buf          (momentum == 0: d = g, momentum_buffer is neither read nor written)
 *     p   = fma(-lr, d, p)
 * "!= 0" is decided on the double the caller passes, as torch decides it on the Python float.
 *
 * Descriptors travel BY VALUE in the kernel arguments (at most 4 KB of explicit arguments per launch; the compiler's hidden arguments come on top): a captured launch owns its pointers,
 * and no device table can go stale under a replay.  The unit of work is a chunk of CSPN_SGD_CHUNK elements of one tensor; the
 * kernel arguments hold the exclusive prefix of chunk counts, a workgroup finds the tensor of a chunk by a uniform binary search
 * and strides over the chunk ids of the launch.  A tensor whose three bases are 16-byte aligned moves 16 bytes at a time, any
 * other tensor (and every tail) element by element: same arithmetic, same bits.  Buffers are aligned to their element size.
 */
#ifndef CSPN_OPTIM_H_
#define CSPN_OPTIM_H_

#include "cspn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CSPN_OPTIM_ABI_VERSION 1

#define CSPN_SGD_CHUNK 4096                /* elements per unit of work: 256 threads x 4 x 16 bytes */
#define CSPN_SGD_TENSORS_PER_LAUNCH 109    /* descriptors + chunk prefix + hyper-parameters of a launch: 4072 of 4096 bytes of explicit arguments */
#define CSPN_SGD_MAX_WORKGROUPS 2048       /* the grid's cap when max_workgroups is 0 (256 .. 8192 measured flat within 2 %) */

/* One tensor of a step: n contiguous fp32 elements each.  momentum_buffer may be NULL when momentum == 0.  first != 0: the
 * tensor's first step with momentum — momentum_buffer is written without being read (it may be uninitialised). */
typedef struct cspn_sgd_tensor_t {
    void* param;
    const void* grad;
    void* momentum_buffer;
    size_t n;
    int first;
} cspn_sgd_tensor_t;

/* One parameter group's hyper-parameters, as the doubles Python holds.  lr_device != NULL: the kernel reads the fp32 rate through
 * it (a DEVICE scalar, read when the launch runs — a captured launch follows it from replay to replay) and `lr` is ignored. */
typedef struct cspn_sgd_hyper_t {
    double lr;
    const float* lr_device;
    double momentum;
    double dampening;
    double weight_decay;
    int nesterov;
    int maximize;
} cspn_sgd_hyper_t;

/* What cspn_sgd_step would launch for tensors of numel[0 .. n_tensors) elements: the number of launches and the number of chunks
 * over all of them (either pointer may be NULL).  Callable without a device.  A tensor of 0 elements takes no descriptor slot.
 * max_workgroups: 0 = CSPN_SGD_MAX_WORKGROUPS; it bounds each launch's grid, min(chunks of the launch, max_workgroups).  A value
 * above 65535 is taken as 65535 (the workgroups stride over the chunks, so a larger grid buys nothing); a negative one fails. */
int cspn_sgd_plan(const size_t* numel, int n_tensors, int max_workgroups, int* launches, size_t* chunks);

/* One step of n_tensors tensors that share `hyper`.  Launches as cspn_sgd_plan says; n_tensors == 0 or all-empty: no launch. */
int cspn_sgd_step(const cspn_sgd_tensor_t* tensors, int n_tensors, const cspn_sgd_hyper_t* hyper, int dtype, int max_workgroups,
                  cspn_stream_t stream);

/* CSPN_OPTIM_ABI_VERSION the library was built from */
int cspn_optim_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CSPN_OPTIM_H_ */
