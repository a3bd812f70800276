/*
 * tcnn_amd.h -- C ABI of libtcnn_amd.so, the MI355X (gfx950) drop-in for tiny-cuda-nn's hot path:
 *     encoding (HashGrid | OneBlob | Identity) -> fully fused fp16 MLP -> loss -> Adam.
 *
 * Every entry point below is what a binding of the reference would bind; the reference interface it replaces is cited
 * as file:line relative to the reference tree (leejaeyong7/tiny-cuda-nn).  Plain pointers and sizes only:
 *   - all data pointers are DEVICE pointers owned by the caller unless stated otherwise;
 *   - "half" buffers are IEEE binary16, passed as void*;
 *   - stream is a hipStream_t passed as void* (NULL = the null stream);
 *   - JSON travels as NUL-terminated UTF-8 text (the reference passes nlohmann::json objects, cpp_api.h:60);
 *   - errors: every int-returning function returns TCNN_OK (0) or TCNN_ERROR and records a message retrievable with
 *     tcnn_last_error() (thread-local).  This replaces the reference's C++ exceptions (common_host.h:71-110).
 *
 * Matrix convention (same memory as the reference): a batch matrix with `w` dims and `n` samples is column-major
 * w x n (gpu_matrix.h:417), i.e. element (dim j, sample i) at ptr[i * w + j]  -- identical to a row-major torch tensor
 * of shape [n, w].  Batch sizes must be multiples of tcnn_batch_size_granularity() = 256 (object.h:130).
 */
#ifndef TCNN_AMD_H
#define TCNN_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCNN_OK 0
#define TCNN_ERROR 1

/* cpp_api.h:69-72 */
#define TCNN_PRECISION_FP32 0
#define TCNN_PRECISION_FP16 1

/* common.h GradientMode */
#define TCNN_GRADIENT_IGNORE 0
#define TCNN_GRADIENT_OVERWRITE 1
#define TCNN_GRADIENT_ACCUMULATE 2

/* common.h:157-162 MatrixLayout: RowMajor == SoA == 0 ([dim][sample]), ColumnMajor == AoS == 1 ([sample][dim]) */
#define TCNN_LAYOUT_SOA 0
#define TCNN_LAYOUT_AOS 1

/* cpp_api.h:52-58 LogSeverity */
#define TCNN_LOG_INFO 0
#define TCNN_LOG_DEBUG 1
#define TCNN_LOG_WARNING 2
#define TCNN_LOG_ERROR 3
#define TCNN_LOG_SUCCESS 4

#define TCNN_MEMCPY_HOST_TO_DEVICE 1
#define TCNN_MEMCPY_DEVICE_TO_HOST 2
#define TCNN_MEMCPY_DEVICE_TO_DEVICE 3

typedef struct tcnn_module_s* tcnn_module_t;       /* tcnn::cpp::Module            cpp_api.h:86-111 */
typedef struct tcnn_context_s* tcnn_context_t;     /* tcnn::cpp::Context           cpp_api.h:82-84  */
typedef struct tcnn_trainer_s* tcnn_trainer_t;     /* tcnn::TrainableModel         config.h:46-51   */
typedef struct tcnn_train_ctx_s* tcnn_train_ctx_t; /* Trainer::ForwardContext      trainer.h:89-95  */
typedef struct tcnn_optimizer_s* tcnn_optimizer_t; /* tcnn::Optimizer<T>            optimizer.h:40-66 */
typedef void* tcnn_stream_t;                       /* hipStream_t */

const char* tcnn_last_error(void);
const char* tcnn_version(void);

/* ---- free functions, cpp_api.h:62-80 / cpp_api.cu:41-63 ---- */
uint32_t tcnn_batch_size_granularity(void);             /* cpp_api.cu:41  */
int      tcnn_device(int* device_out);                  /* cpp_api.cu:43  cuda_device() */
int      tcnn_set_device(int device);                   /* cpp_api.cu:44  set_cuda_device() */
void     tcnn_free_temporary_memory(void);              /* cpp_api.cu:45  */
int      tcnn_has_networks(void);                       /* cpp_api.cu:47  */
float    tcnn_default_loss_scale(int precision);        /* cpp_api.cu:55  */
int      tcnn_preferred_precision(void);                /* cpp_api.cu:60  */
void     tcnn_set_log_callback(void (*callback)(int severity, const char* message, void* user), void* user); /* cpp_api.cu:61 */

/* ---- device memory and stream helpers for callers that do not link the HIP runtime themselves: what GPUMemory<T>
 * (gpu_memory.h:60-392) and GPUMatrix<T> (gpu_matrix.h:417-470) need from a runtime; used by include/tiny-cuda-nn/ ---- */
int tcnn_gpu_malloc(size_t bytes, void** out);                              /* gpu_memory.h:93-112  allocate_memory */
int tcnn_gpu_free(void* ptr);                                               /* gpu_memory.h:114-130 free_memory */
int tcnn_gpu_memcpy(void* dst, const void* src, size_t bytes, int kind);    /* gpu_memory.h:183-260 copy_from_host / copy_to_host */
int tcnn_gpu_memset(void* ptr, int value, size_t bytes);                    /* gpu_memory.h:171-181 memset */
int tcnn_stream_synchronize(tcnn_stream_t stream);
/* random.h:58-70 generate_random_uniform<float>(stream, rng, n, out, lower, upper): thread i of the reference's kernel advances a
 * copy of the pcg32 by 4 i and writes elements i + n_threads j (j < 4); the caller's generator is then advanced by n.
 * rng_state_inc = {state, inc} of a pcg32 (include/tiny-cuda-nn/random.h keeps them), updated in place. */
int tcnn_generate_random_uniform(tcnn_stream_t stream, uint64_t rng_state_inc[2], size_t n, float* out, float lower, float upper);

/* ---- factories, cpp_api.h:113-115 / cpp_api.cu:146-165.  The caller owns the returned module. ---- */
int  tcnn_create_network_with_input_encoding(uint32_t n_input_dims, uint32_t n_output_dims, const char* encoding_json, const char* network_json, tcnn_module_t* out);
int  tcnn_create_network(uint32_t n_input_dims, uint32_t n_output_dims, const char* network_json, tcnn_module_t* out);
int  tcnn_create_encoding(uint32_t n_input_dims, const char* encoding_json, int precision, tcnn_module_t* out);
/* The two network factories with the module's precision as an argument (TCNN_PRECISION_*; the two above are the FP16 case).  FP32 is the
 * reference's build without TCNN_HALF_PRECISION as a choice per module: the encoding in its fp32 form in front of a CutlassMLP<float>
 * that runs layer by layer.  params, output, dL_doutput, dL_dparams and dL_ddLdoutput of such a module are float, and
 * tcnn_module_param_precision / tcnn_module_output_precision answer TCNN_PRECISION_FP32 (tcnn_preferred_precision() stays FP16).  "otype":
 * "FullyFusedMLP" with FP32 reports "FullyFusedMLP can only be used if the network precision is set to __half." (network.cu:102-103). */
int  tcnn_create_network_with_input_encoding_precision(uint32_t n_input_dims, uint32_t n_output_dims, const char* encoding_json, const char* network_json, int precision, tcnn_module_t* out);
int  tcnn_create_network_precision(uint32_t n_input_dims, uint32_t n_output_dims, const char* network_json, int precision, tcnn_module_t* out);
void tcnn_module_destroy(tcnn_module_t module);

/* ---- Module methods, cpp_api.h:91-106 / cpp_api.cu:72-139 ----
 * input [n][n_input_dims] float; output / dL_doutput [n][n_output_dims()] in output_precision (n_output_dims() is the PADDED
 * width, cpp_api.cu:130); params: ONE flat vector in param_precision, network weights first, then encoding parameters
 * (network_with_input_encoding.h:115-122), re-bound on every call.  dL_dparams == NULL => GradientMode::Ignore, else Overwrite. */
int  tcnn_module_inference(tcnn_module_t m, tcnn_stream_t stream, uint32_t n_elements, const float* input, void* output, void* params);
int  tcnn_module_forward(tcnn_module_t m, tcnn_stream_t stream, uint32_t n_elements, const float* input, void* output, void* params,
                         int prepare_input_gradients, tcnn_context_t* ctx_out);
int  tcnn_module_backward(tcnn_module_t m, tcnn_stream_t stream, tcnn_context_t ctx, uint32_t n_elements, float* dL_dinput,
                          const void* dL_doutput, void* dL_dparams, const float* input, const void* output, const void* params);
/* second-order input gradients (cpp_api.h:94, cpp_api.cu:111-127; grid.h:902-1026): dL_ddLdinput [n][n_input_dims] float is the
 * gradient arriving at dL_dinput; optional results dL_dparams (Overwrite), dL_ddLdoutput [n][n_output_dims], dL_dinput [n][n_input_dims]
 * (overwritten; the reference adds into a zeroed buffer).  The context must come from tcnn_module_forward(prepare_input_gradients = 1).
 * Modules that implement it: the grid encodings, PPNG3, Identity, Frequency, TriangleWave, SphericalHarmonics, Empty and a Composite of
 * those (Concatenation, Sum or Product); networks of otype CutlassMLP / MLP (every width, depth and activation the constructor accepts),
 * alone (tcnn_create_network) or behind one of those encodings.  FullyFusedMLP does not, as in the reference: ask for "otype":
 * "CutlassMLP", whose first-order passes still run the fused kernels for the shapes those cover.  It, OneBlob, PPNG1 / PPNG2 and a
 * Composite that holds one of them (OneBlobFrequency / NRC) report "DifferentiableObject::backward_backward_input_impl: not implemented
 * error" (object.h:288) before anything is allocated or launched. */
int  tcnn_module_backward_backward_input(tcnn_module_t m, tcnn_stream_t stream, tcnn_context_t ctx, uint32_t n_elements, const float* dL_ddLdinput,
                                         const float* input, const void* dL_doutput, void* dL_dparams, void* dL_ddLdoutput, float* dL_dinput, const void* params);
/* the same with an explicit TCNN_GRADIENT_* mode for dL_dparams (ACCUMULATE adds onto what the buffer holds; IGNORE: dL_dparams unused) */
int  tcnn_module_backward_backward_input_mode(tcnn_module_t m, tcnn_stream_t stream, tcnn_context_t ctx, uint32_t n_elements, const float* dL_ddLdinput,
                                              const float* input, const void* dL_doutput, void* dL_dparams, void* dL_ddLdoutput, float* dL_dinput, const void* params,
                                              int gradient_mode);
/* DifferentiableObject::input_gradient (object.h:342-366): d_dinput [n_elements][n_input_dims] = d output[dim] / d input with `params`, at
 * inference -- no parameter gradient is read or written and no context is left.  dim counts the PADDED output columns (a padded column is
 * legal); dim >= tcnn_module_n_output_dims reports "Invalid dimension to compute the input gradient for." before anything is allocated or
 * launched, and n_elements must be a multiple of tcnn_batch_size_granularity().  The result is what forward(prepare_input_gradients) +
 * backward with dL_doutput = (output precision)backprop_scale in column dim and +0 elsewhere give, multiplied by the float 1.0f /
 * backprop_scale -- bit for bit, whichever route ran.  output (may be NULL): [n_elements][n_output_dims] in the output precision, the
 * forward pass's output.  A grid encoding's max_level state applies as in any forward pass. */
int  tcnn_module_input_gradient(tcnn_module_t m, tcnn_stream_t stream, uint32_t n_elements, uint32_t dim, const float* input, float* d_dinput, void* output,
                                const void* params, float backprop_scale);
/* Introspection: the route the module's last input_gradient call took -- "none" before the first call, "two-pass" (forward + backward
 * kernels) or the fused MLP kernel's name, "k_mlp_input_grad<W,NB,NH>/relu|act" (/act: the hidden activation is chosen at run time).
 * Owned by the module: valid until its next input_gradient call.  NULL (and tcnn_last_error) for a NULL module. */
const char* tcnn_module_last_input_gradient_route(tcnn_module_t m);
/* input_gradient for n_dims output columns from ONE forward pass: jacobian [n_elements][n_dims][n_input_dims] floats, row-major.  For
 * every k, rows [:, k, :] are bit for bit what tcnn_module_input_gradient(dim = dims[k]) returns for the same input, params, backprop_scale
 * and max_level state, and output (may be NULL) is bit for bit its output -- whichever route either call takes.  dims is a HOST array of
 * n_dims padded output columns, in any order, repeats allowed; 1 <= n_dims <= tcnn_module_n_output_dims.  Checked before anything is
 * allocated or launched: NULL dims or an n_dims outside that range (a message that names n_dims), a dim >= tcnn_module_n_output_dims
 * ("Invalid dimension to compute the input gradient for."), n_elements off tcnn_batch_size_granularity(). */
int  tcnn_module_input_jacobian(tcnn_module_t m, tcnn_stream_t stream, uint32_t n_elements, const uint32_t* dims, uint32_t n_dims, const float* input, float* jacobian,
                                void* output, const void* params, float backprop_scale);
/* The route the module's last input_jacobian call took: "none" before the first call, "two-pass" (one forward pass, n_dims backward passes)
 * or the fused MLP kernel's name, "k_mlp_input_jacobian<W,NB,NH>/relu|act".  Owned by the module, as tcnn_module_last_input_gradient_route. */
const char* tcnn_module_last_input_jacobian_route(tcnn_module_t m);
/* Forward mode, the opposite question: how do ALL outputs change when the input moves along a direction v.  tangents [n_elements][n_tangents]
 * [n_input_dims] floats, row-major, n_tangents >= 1; jvp [n_elements][n_tangents][tcnn_module_n_output_dims] in the module's OUTPUT
 * precision (tcnn_module_output_precision), row-major: jvp[:, t, :] = J(x) tangents[:, t, :] -- d/dt of every feature of a 4-D field, grad f . d
 * along a ray, a 3 x 3 (or n_out x 3) deformation Jacobian from three directions.  Runs at inference: no parameter gradient is read or written
 * and no context is left; a grid encoding's max_level state applies as in any forward pass.  output (may be NULL), [n_elements]
 * [tcnn_module_n_output_dims] in the output precision, is bit for bit what tcnn_module_inference returns.  Padded output columns hold what the
 * second-order pass puts there.  On the route "two-pass" -- one forward pass with input gradients prepared, then per direction the
 * encoding's tangent and the network's layer-by-layer tangent pass -- jvp[:, t, :] is bit for bit the dL_ddLdoutput that tcnn_module_forward
 * (prepare_input_gradients = 1) + tcnn_module_backward_backward_input(dL_ddLdinput = tangents[:, t, :]) return, for every module that has that
 * pass; FullyFusedMLP networks and OneBlob encodings, which have none, have tangents all the same.  There is NO backprop_scale: the map is linear
 * in v, so a caller who fears overflow in half precision scales v and divides the result.  Checked before anything is allocated or
 * launched: NULL tangents or jvp, n_tangents == 0 (a message that names n_tangents), n_elements off tcnn_batch_size_granularity(), and a module
 * without a tangent -- PPNG1, PPNG2 or a Composite holding one: "input_jvp: not implemented for <module name>".  A refused call leaves the
 * route strings alone. */
int  tcnn_module_input_jvp(tcnn_module_t m, tcnn_stream_t stream, uint32_t n_elements, uint32_t n_tangents, const float* input, const float* tangents, void* jvp, void* output,
                           const void* params);
/* The route the module's last input_jvp call took: "none" before the first call, "two-pass", or the fused MLP kernel's name,
 * "k_mlp_input_jvp<W,NB,NH,TT>/relu|act" (TT: tangent chains per launch).  Owned by the module, as tcnn_module_last_input_gradient_route. */
const char* tcnn_module_last_input_jvp_route(tcnn_module_t m);
/* Training through input_jvp: the pair below puts J v into a loss.  tcnn_module_input_jvp_forward is tcnn_module_input_jvp -- the same route,
 * the same bits in jvp and output (output may be NULL), the same refusals -- and returns a context for tcnn_module_input_jvp_backward
 * (destroy it with tcnn_context_destroy; it holds no device memory: the backward call runs the module's forward pass again from input).
 * tcnn_module_input_jvp_backward gives the gradients of
 *     L = sum_t <dL_djvp[:, t, :], J(input) tangents[:, t, :]> + <dL_doutput, f(input)>
 * for dL_djvp [n_elements][n_tangents][padded output width] and dL_doutput [n_elements][padded output width] (may be NULL) in the module's
 * output precision, taken as they are: there is no loss scale inside.  Results, each may be NULL and only what is asked for is computed:
 * dL_dparams [n_params] in the parameters' precision under gradient_mode (TCNN_GRADIENT_*, as tcnn_module_backward_backward_input_mode),
 * dL_dinput [n_elements][n_input_dims] and dL_dtangents [n_elements][n_tangents][n_input_dims] floats.  First order only.  input, tangents
 * and params are those of the forward call.  On the route "two-pass" the call is composed of the module's existing passes -- one forward
 * pass with input gradients prepared; the backward pass of dL_doutput, if there is one; then per tangent the second-order pass (dL_ddLdinput =
 * tangents[:, t, :], dL_doutput = dL_djvp[:, t, :]) for dL_dparams and dL_dinput and a first-order backward pass for dL_dtangents[:, t, :] -- and
 * every result is bit for bit what a caller gets who chains tcnn_module_forward / _backward / _backward_backward_input_mode by hand in that
 * order, accumulating dL_dparams through TCNN_GRADIENT_ACCUMULATE and adding the dL_dinput terms in fp32 (a grid's second-order parameter
 * gradients: up to the order of its atomic additions).  FullyFusedMLP networks and OneBlob
 * encodings, whose tcnn_module_backward_backward_input stays refused, are served here.  A grid's max_level state in force applies to both
 * calls.  Checked before anything is allocated or launched, a refused call leaving the route strings alone: what tcnn_module_input_jvp
 * checks (NULL tangents or dL_djvp, n_tangents == 0, n_elements off the granularity, a module without a tangent: "input_jvp: not implemented
 * for <module name>"); a context that is not one of tcnn_module_input_jvp_forward ("Module::bwd: called with invalid context. ..."), or of a call
 * with another n_elements or n_tangents; dL_dinput behind an encoding whose tangent has no derivative by x here -- OneBlob, or a Composite
 * holding one: "input_jvp_backward: dL_dinput not implemented for <module name>" (dL_dparams and dL_dtangents work there; dL_dparams is refused
 * likewise only if such a Composite has parameters of its own). */
int  tcnn_module_input_jvp_forward(tcnn_module_t m, tcnn_stream_t stream, uint32_t n_elements, uint32_t n_tangents, const float* input, const float* tangents, void* jvp,
                                   void* output, const void* params, tcnn_context_t* ctx_out);
int  tcnn_module_input_jvp_backward(tcnn_module_t m, tcnn_stream_t stream, tcnn_context_t ctx, uint32_t n_elements, uint32_t n_tangents, const float* input,
                                    const float* tangents, const void* dL_djvp, const void* dL_doutput, const void* params, void* dL_dparams, float* dL_dinput,
                                    float* dL_dtangents, int gradient_mode);
/* The route the module's last input_jvp_backward call took: "none" before the first call, "two-pass" (the composed route; a fused kernel's
 * name, "k_mlp_input_jvp_bwd<W,NB,NH,TT>/relu|act", is reserved for one that is measured faster).  Owned by the module. */
const char* tcnn_module_last_input_jvp_backward_route(tcnn_module_t m);
void tcnn_context_destroy(tcnn_context_t ctx);

uint32_t    tcnn_module_n_input_dims(tcnn_module_t m);     /* cpp_api.cu:129 */
uint32_t    tcnn_module_n_output_dims(tcnn_module_t m);    /* cpp_api.cu:130 (padded) */
size_t      tcnn_module_n_params(tcnn_module_t m);         /* cpp_api.cu:131 */
int         tcnn_module_param_precision(tcnn_module_t m);  /* cpp_api.h:103 */
int         tcnn_module_output_precision(tcnn_module_t m); /* cpp_api.h:100 */
/* cpp_api.cu:133-136: pcg32 rng{seed}; fills params_full_precision (device, float[n_params]) */
int         tcnn_module_initialize_params(tcnn_module_t m, uint64_t seed, float* params_full_precision, float scale);
const char* tcnn_module_hyperparams(tcnn_module_t m);      /* JSON text owned by the module; cpp_api.cu:138 */
const char* tcnn_module_name(tcnn_module_t m);             /* cpp_api.cu:139 */

/* ---- boundary A: create_from_config / Trainer (config.h:53-63, trainer.h:48-363) ---- */
int  tcnn_create_from_config(uint32_t n_input_dims, uint32_t n_output_dims, const char* config_json, tcnn_trainer_t* out);          /* seed 1337, trainer.h:50 */
int  tcnn_create_from_config_seeded(uint32_t n_input_dims, uint32_t n_output_dims, const char* config_json, uint32_t seed, tcnn_trainer_t* out);
/* The trainer's precision as an argument (TCNN_PRECISION_*; the two factories above are the FP16 case).  FP32 is Trainer<float, float, float>
 * of the reference's build without TCNN_HALF_PRECISION: the fp32 module (tcnn_create_network_with_input_encoding_precision), the loss on float
 * predictions, an optimizer with fp32 weights, loss scale tcnn_default_loss_scale(TCNN_PRECISION_FP32) = 1.  Such a trainer has ONE float
 * parameter vector -- tcnn_trainer_params == tcnn_trainer_params_full_precision -- and every training_step is the unfused sequence
 * (tcnn_trainer_last_step_kernel: "unfused").  Every pointer typed void* below -- tcnn_trainer_params, _params_inference, _param_gradients,
 * tcnn_train_ctx_output, _dL_doutput -- points at elements of the trainer's precision; tcnn_trainer_set_params and external_dL_dy take that
 * precision, and tcnn_trainer_inference_mixed_precision writes it.  The initial parameters are the same floats for either precision and the
 * same seed.  Configuration errors ("FullyFusedMLP can only be used if the network precision is set to __half.", an invalid loss or
 * optimizer type, "Unknown precision N") are reported before anything is allocated on the device. */
int  tcnn_create_from_config_precision(uint32_t n_input_dims, uint32_t n_output_dims, const char* config_json, uint32_t seed, int precision, tcnn_trainer_t* out);
int  tcnn_trainer_precision(tcnn_trainer_t t);                    /* TCNN_PRECISION_*; -1 + tcnn_last_error() for a NULL handle */
void tcnn_trainer_destroy(tcnn_trainer_t t);

/* Trainer::training_step (trainer.h:163-190).  input: float, n_input_dims x n in `input_layout`; target: float [n][n_output_dims];
 * data_pdf (optional) like target; dL_dinput (optional) float in input_layout; external_dL_dy (optional) [n][padded_out] in the trainer's
 * precision (half, or float for an FP32 trainer).
 * Returns the forward context (caller destroys it) -- loss is fetched with tcnn_trainer_loss like trainer->loss(stream, *ctx). */
int  tcnn_trainer_training_step(tcnn_trainer_t t, tcnn_stream_t stream, uint32_t n_elements, const float* input, int input_layout,
                                const float* target, const float* data_pdf, int run_optimizer, float* dL_dinput, int use_inference_params,
                                int gradient_mode, const void* external_dL_dy, tcnn_train_ctx_t* ctx_out);
/* Trainer::loss (trainer.h:205-207): sum of the per-element loss values; synchronises the stream */
int  tcnn_trainer_loss(tcnn_trainer_t t, tcnn_stream_t stream, tcnn_train_ctx_t ctx, float* loss_out);
/* the three pieces of a step, trainer.h:97-157 */
int  tcnn_trainer_forward(tcnn_trainer_t t, tcnn_stream_t stream, float loss_scale, uint32_t n_elements, const float* input, int input_layout, const float* target,
                          const float* data_pdf, int use_inference_params, int prepare_input_gradients, const void* external_dL_dy, tcnn_train_ctx_t* ctx_out);
int  tcnn_trainer_backward(tcnn_trainer_t t, tcnn_stream_t stream, tcnn_train_ctx_t ctx, uint32_t n_elements, const float* input, int input_layout,
                           float* dL_dinput, int use_inference_params, int gradient_mode);
int  tcnn_trainer_optimizer_step(tcnn_trainer_t t, tcnn_stream_t stream, float loss_scale);
void tcnn_train_ctx_destroy(tcnn_train_ctx_t ctx);
/* ForwardContext members (trainer.h:89-95): device pointers valid until the context is destroyed.
 * The fused training step keeps dL_doutput and L as dense [n][n_output_dims] matrices (the padding columns are zeros) and forms
 * the padded ones on the FIRST call of their accessor, on the step's stream. */
const void*  tcnn_train_ctx_output(tcnn_train_ctx_t ctx);      /* half  [n][padded_out] (float from an FP32 trainer) */
const void*  tcnn_train_ctx_dL_doutput(tcnn_train_ctx_t ctx);  /* half  [n][padded_out] (float from an FP32 trainer); NULL + tcnn_last_error() on failure */
const float* tcnn_train_ctx_L(tcnn_train_ctx_t ctx);           /* float [n][padded_out]; NULL + tcnn_last_error() on failure */

/* network->inference(stream, input, output) (object.h:147-176): float in, float out [n_output_dims x n] in output_layout */
int  tcnn_trainer_inference(tcnn_trainer_t t, tcnn_stream_t stream, uint32_t n_elements, const float* input, int input_layout,
                            float* output, int output_layout, int use_inference_params);
/* network->input_gradient(stream, dim, input, d_dinput, backprop_scale) (object.h:342-366) on the trainer's inference parameters: see
 * tcnn_module_input_gradient.  input and d_dinput are AoS [n_elements][n_input_dims] floats. */
int  tcnn_trainer_input_gradient(tcnn_trainer_t t, tcnn_stream_t stream, uint32_t n_elements, uint32_t dim, const float* input, float* d_dinput, float backprop_scale);
/* tcnn_module_input_jacobian on the trainer's inference parameters: jacobian [n_elements][n_dims][n_input_dims] floats; dims is a host array */
int  tcnn_trainer_input_jacobian(tcnn_trainer_t t, tcnn_stream_t stream, uint32_t n_elements, const uint32_t* dims, uint32_t n_dims, const float* input, float* jacobian,
                                 float backprop_scale);
/* tcnn_module_input_jvp on the trainer's inference parameters: tangents [n_elements][n_tangents][n_input_dims] floats, jvp [n_elements][n_tangents]
 * [padded output width] in the trainer's precision */
int  tcnn_trainer_input_jvp(tcnn_trainer_t t, tcnn_stream_t stream, uint32_t n_elements, uint32_t n_tangents, const float* input, const float* tangents, void* jvp);
/* tcnn_module_input_jvp_forward / _backward on the trainer's TRAINING parameters; the parameter gradients go into the trainer's gradient buffer
 * under gradient_mode, where tcnn_trainer_optimizer_step reads them (cotangents scaled by a loss scale give gradients scaled by it) */
int  tcnn_trainer_input_jvp_forward(tcnn_trainer_t t, tcnn_stream_t stream, uint32_t n_elements, uint32_t n_tangents, const float* input, const float* tangents, void* jvp,
                                    void* output, tcnn_context_t* ctx_out);
int  tcnn_trainer_input_jvp_backward(tcnn_trainer_t t, tcnn_stream_t stream, tcnn_context_t ctx, uint32_t n_elements, uint32_t n_tangents, const float* input,
                                     const float* tangents, const void* dL_djvp, const void* dL_doutput, float* dL_dinput, float* dL_dtangents, int gradient_mode);

/* network->inference_mixed_precision(stream, input, output) (object.h:133-145): the network's own output, half
 * [n_elements][padded_output_width] -- what inference() casts to float; half the bytes for a caller that gathers row shards.
 * An FP32 trainer writes floats. */
int  tcnn_trainer_inference_mixed_precision(tcnn_trainer_t t, tcnn_stream_t stream, uint32_t n_elements, const float* input, int input_layout,
                                            void* output_half, int use_inference_params);

size_t   tcnn_trainer_n_params(tcnn_trainer_t t);                 /* trainer.h:338 */
uint32_t tcnn_trainer_padded_output_width(tcnn_trainer_t t);
float*   tcnn_trainer_params_full_precision(tcnn_trainer_t t);    /* trainer.h:226 */
void*    tcnn_trainer_params(tcnn_trainer_t t);                   /* trainer.h:230 (half; an FP32 trainer: its float vector, = params_full_precision) */
void*    tcnn_trainer_params_inference(tcnn_trainer_t t);         /* trainer.h:234 */
void*    tcnn_trainer_param_gradients(tcnn_trainer_t t);          /* trainer.h:238 (half; float for an FP32 trainer) */
int      tcnn_trainer_set_params_full_precision(tcnn_trainer_t t, const float* params, size_t n_params, int device_ptr); /* trainer.h:242 */
int      tcnn_trainer_set_params(tcnn_trainer_t t, const void* params_half, size_t n_params, int device_ptr);            /* trainer.h:256 (floats for an FP32 trainer) */
int      tcnn_trainer_initialize_params(tcnn_trainer_t t);        /* trainer.h:68-87 (re-initialise, continues the rng stream) */
int      tcnn_trainer_update_hyperparams(tcnn_trainer_t t, const char* json); /* trainer.h:213 */
const char* tcnn_trainer_hyperparams(tcnn_trainer_t t);           /* trainer.h:218; JSON text owned by the trainer */
/* Snapshot wire format, trainer.h:275-315 (json serialize(bool) / deserialize(const json&)) with adam.h:278-299 and
 * gpu_memory_json.h:36-71: the object {"n_params", "params_type": "__half", "params_binary": <bin>, ["optimizer":
 * {"current_step", "base_learning_rate", "first_moments_binary", "second_moments_binary", "param_steps_binary"}]} as
 * MessagePack bytes, encoded the way nlohmann::json::to_msgpack encodes it (what instant-ngp-style callers write to disk).
 * serialize: the buffer belongs to the trainer and stays valid until its next serialize call or its destruction.
 * An FP32 trainer writes "params_type": "float" and 4 n_params bytes, and the custom-weight blobs of its optimizer (Ema, Average, Lookahead)
 * hold floats.
 * deserialize: accepts "params_type" "__half" or "float" in a trainer of either precision (cast as trainer.h:296-305 does), binary values or
 * their text form {"bytes": [...]}.  Optimizer state whose blobs are of the other weight precision is an error, never reinterpreted. */
int      tcnn_trainer_serialize(tcnn_trainer_t t, int serialize_optimizer, const void** out_bytes, size_t* out_size);
int      tcnn_trainer_deserialize(tcnn_trainer_t t, const void* bytes, size_t size);
const char* tcnn_trainer_network_hyperparams(tcnn_trainer_t t);   /* network->hyperparams() */
uint32_t tcnn_trainer_optimizer_step_count(tcnn_trainer_t t);     /* optimizer->step() adam.h:198 */
/* Measurement hook (no counterpart in the reference; bench.py): the NEXT fused training_step() records HIP events on
 * its stream around its pieces -- [0] encoding forward, [1] the fused MLP kernel (forward + loss + backward + weight gradients),
 * [2] encoding backward, [3] optimizer.  _collect synchronises the stream and returns the milliseconds per piece summed over the
 * steps profiled since the last call, and their number. */
int  tcnn_trainer_profile_next_step(tcnn_trainer_t t);
int  tcnn_trainer_profile_collect(tcnn_trainer_t t, tcnn_stream_t stream, float* ms_per_piece /* [4] */, uint32_t* n_steps);
/* Introspection (no counterpart in the reference): how many parameters of the last training_step() had their optimizer update
 * applied by the launch that finished their gradients -- the reduction of the network's weight gradients -- instead of by the
 * optimizer kernel.  Either every parameter or none: n_params for a fused step with run_optimizer=true, plain Adam, GradientMode
 * Overwrite, a model without encoding parameters and no dL_dinput asked for (TCNN_AMD_ADAM_IN_REDUCE=0 turns it off), else 0. */
size_t tcnn_trainer_params_updated_in_flush(tcnn_trainer_t t);
/* Introspection (no counterpart in the reference): how many times training_step() calls of this trainer have launched the kernel
 * that rearranges the network's weights into matrix-instruction fragments.  A model without encoding parameters trained with plain
 * Adam keeps those fragments current from inside its optimizer kernel, so the count stops growing after the first step -- until
 * the parameters are set, restored, stepped by optimizer_step(), or a pointer to them has been handed out
 * (tcnn_trainer_params / tcnn_trainer_params_full_precision: from then on every step rearranges them again). */
size_t tcnn_trainer_image_preps(tcnn_trainer_t t);
/* Introspection (no counterpart in the reference): the grid encoding's gradient kernel (replacing kernel_grid_backward, grid.h:215-320)
 * sums a chunk's fp16 products as exact integers, two 32-bit sums per 64-bit LDS add while a per-task bound on sum |product| proves
 * that neither can overflow; a task whose bound fails runs again with 64-bit sums (same result, slower).  This counts those tasks since
 * the trainer was built; (size_t)-1 on error.  Synchronises with the device. */
size_t tcnn_trainer_scatter_wide_fallbacks(tcnn_trainer_t t);
/* Introspection (no counterpart in the reference): training steps of this trainer whose optimizer launch (adam_step, adam.h:150-188)
 * also ran the last two reductions of the backward pass -- the rounding of the grid gradient's shared chunks and the sum of the network's
 * weight-gradient slabs -- instead of a launch of their own in front of it (same results; TCNN_AMD_ADAM_PROLOGUE=0 separates them). */
size_t tcnn_trainer_optimizer_prologue_steps(tcnn_trainer_t t);
/* Introspection (no counterpart in the reference): backward passes of this trainer's grid encoding that ran the list-fed gradient
 * kernel (k_grid_scatter_lists: hit lists written by the forward kernel) rather than the bit-plane, binned or atomic forms -- tests assert
 * which kernel produced the gradients they compare with the oracle (replaces kernel_grid_backward, grid.h:215-320). */
size_t tcnn_trainer_list_scatters(tcnn_trainer_t t);
size_t tcnn_module_list_scatters(tcnn_module_t m); /* the same count for a module's grid encoding(s) (callers with their own network) */
/* Introspection (no counterpart in the reference): training steps of this trainer whose fused MLP kernel also stored dL/d(encoding) in
 * the order of the grid encoding's hit lists, as its tail, instead of a k_grid_list_gradients launch in front of the list-fed gradient
 * kernel (same results; TCNN_AMD_LISTGRAD_IN_MLP=0 keeps the separate launch). */
size_t tcnn_trainer_list_gradient_tails(tcnn_trainer_t t);
/* Introspection (no counterpart in the reference): a short, stable name of the MLP training kernel the last training_step() of this
 * trainer launched -- "r32", "r32a", "r32w", "r32ob", "regs_fast", "regs", "train<W,NB,NW,MAXT>/relu", "train<W,NB,NW,MAXT>/act",
 * "train_regw/...", "train_ob/..." (/act: the hidden activation is chosen at run time) or "unfused"
 * (forward, loss, backward and weight-gradient kernels of their own); "" before the first step.  A static string: do not free it. */
const char* tcnn_trainer_last_step_kernel(tcnn_trainer_t t);

/* max_level of the grid encodings (GridEncoding::set_max_level / max_level / set_max_level_gpu / max_level_gpu, grid_interface.h:101-123):
 * a fraction of the levels, 1000 (the default) keeps every one.  With m = max_level * n_levels, level l produces zeros (in its features and
 * in the input gradients) when l >= m + 1e-3f, and receives no parameter gradient when l > m + 1e-3f (grid.h:67-90, :237-245, :377-384,
 * :482-490; fp32 arithmetic, NaN keeps every level on).  A skipped level's gradients are zero under Overwrite and untouched under
 * Accumulate; the optimizer still steps those parameters.  Every grid nested in the module (Composite) takes the setting, which is read
 * when each call runs and is neither part of the hyperparameters nor of snapshots.
 * per_sample: device memory the caller owns, one float per row, read instead of the scalar (NULL: the scalar again).  It must hold at
 * least n_elements floats for EVERY call made on the module / trainer while it is set, and stay valid until those calls have run.
 * A module or trainer without a grid encoding: TCNN_ERROR, or NaN from the getters, and tcnn_last_error() names the model; a getter that
 * succeeds leaves tcnn_last_error() empty (which tells a NaN that was set from an error). */
int   tcnn_module_set_max_level(tcnn_module_t m, float max_level);
float tcnn_module_max_level(tcnn_module_t m);
int   tcnn_module_set_max_level_gpu(tcnn_module_t m, const float* per_sample);
/* the trainer's model: training_step, forward / backward and both inference calls */
int   tcnn_trainer_set_max_level(tcnn_trainer_t t, float max_level);
int   tcnn_trainer_set_max_level_gpu(tcnn_trainer_t t, const float* per_sample);
float tcnn_trainer_max_level(tcnn_trainer_t t);
/* Introspection: 1 when this context owns the network's weight-gradient slabs because their reduction was left to the optimizer's
 * launch (tcnn_trainer_optimizer_prologue_steps): they must outlive training_step()'s own scope, until that launch is enqueued. */
int tcnn_train_ctx_keeps_weight_gradient_slabs(tcnn_trainer_t t, tcnn_train_ctx_t ctx);


/* ---- standalone optimizers (optimizer.h:44-95, src/optimizer.cu:50-82): the optimizers a trainer runs, for callers that compute the
 * gradients themselves -- Adam, SGD, Novograd, Ema, ExponentialDecay, Average, Batched, Lookahead, Composite, nested as in a trainer's
 * "optimizer" configuration.
 * tcnn_module_layer_sizes: the (rows, cols) of the module's weight matrices in parameter order -- what Optimizer::allocate takes beside
 * n_params (matrix weights come first in the parameter vector; Adam's l2_reg and non_matrix_learning_rate_factor, Novograd's layers and
 * Composite's slices go by them).  Writes min(n_layers, capacity) pairs into rows_cols and the full count into *n_layers_out.
 * tcnn_optimizer_create: the configuration is checked before anything is allocated ("Invalid optimizer type: ..." needs no device);
 * layer_sizes holds n_layers (rows, cols) pairs.
 * tcnn_optimizer_step: one step on `stream`.  params_full_precision float[n_params] and params_half half[n_params] are the caller's:
 * the fp32 master weights and the half working copy, both updated (a non-matrix parameter whose gradient is zero keeps both, adam.h:76-84).
 * gradients: n_params values in gradient_precision -- TCNN_PRECISION_FP16, scaled by loss_scale like a trainer's, or TCNN_PRECISION_FP32
 * (a caller's own, e.g. a PyTorch .grad: loss_scale 1 when they are unscaled already).  Both forms run the same arithmetic on the unscaled
 * value; fp32 gradients are not rounded to half anywhere (Batched hands its fp32 mean to the nested optimizer as it is).
 * serialize / deserialize: the MessagePack bytes of the object a trainer's snapshot carries as its "optimizer" entry (tcnn_trainer_serialize),
 * so the two are interchangeable; the buffer belongs to the handle until its next serialize call or its destruction.  Both synchronise
 * with the device.
 * custom_weights: half[n_params] the optimizer keeps for inference (Ema, Average, Lookahead; Composite when a nested one has any), or NULL.
 * The getters return 0 / NaN / NULL and leave a message in tcnn_last_error() when given a NULL handle.
 * weights_restored: call after overwriting params_half by other means, and after deserialize (optimizers that assemble their custom
 * weights from several sources -- Composite -- rebuild them from params_half; a snapshot does not carry them).
 * tcnn_optimizer_create_precision: the weights' precision as an argument (tcnn_optimizer_create is the FP16 case).  TCNN_PRECISION_FP32 is
 * Optimizer<float>: ONE float weight vector -- the master vector is the working vector, read and stored once per step.  tcnn_optimizer_step
 * then takes params_half == NULL or == params_full_precision and gradient_precision == TCNN_PRECISION_FP32 (anything else is an error);
 * custom_weights points at float[n_params]; weights_restored takes the float vector; the snapshot's custom-weight blobs hold floats, and a
 * blob of another size than n_params elements of the optimizer's weight precision is an error.  The master-weight arithmetic is the same:
 * Adam, SGD, Novograd, ExponentialDecay, Batched and a Composite of those leave master weights, moments and step counts bit-identical to
 * the FP16-weight optimizer stepped on the same fp32 gradients.  "Unknown precision N" for any other value. */
int         tcnn_module_layer_sizes(tcnn_module_t m, uint32_t* rows_cols, size_t capacity, size_t* n_layers_out);
int         tcnn_optimizer_create(const char* optimizer_json, size_t n_params, const uint32_t* layer_sizes, size_t n_layers, tcnn_optimizer_t* out);
int         tcnn_optimizer_create_precision(const char* optimizer_json, size_t n_params, const uint32_t* layer_sizes, size_t n_layers, int weight_precision, tcnn_optimizer_t* out);
int         tcnn_optimizer_weight_precision(tcnn_optimizer_t o);                                /* TCNN_PRECISION_*; -1 + tcnn_last_error() for a NULL handle */
void        tcnn_optimizer_destroy(tcnn_optimizer_t o);
int         tcnn_optimizer_step(tcnn_optimizer_t o, tcnn_stream_t stream, float loss_scale, float* params_full_precision, void* params_half,
                                const void* gradients, int gradient_precision);                 /* optimizer.h:49 */
uint32_t    tcnn_optimizer_step_count(tcnn_optimizer_t o);                                      /* optimizer.h:52 step() */
size_t      tcnn_optimizer_n_params(tcnn_optimizer_t o);                                        /* optimizer.h:53 n_weights() */
float       tcnn_optimizer_learning_rate(tcnn_optimizer_t o);                                   /* optimizer.h:50 */
int         tcnn_optimizer_set_learning_rate(tcnn_optimizer_t o, float learning_rate);          /* optimizer.h:51 */
int         tcnn_optimizer_update_hyperparams(tcnn_optimizer_t o, const char* json);
const char* tcnn_optimizer_hyperparams(tcnn_optimizer_t o);                                     /* JSON text owned by the handle */
void*       tcnn_optimizer_custom_weights(tcnn_optimizer_t o);                                  /* optimizer.h:54 */
int         tcnn_optimizer_weights_restored(tcnn_optimizer_t o, tcnn_stream_t stream, const void* params_half);
int         tcnn_optimizer_serialize(tcnn_optimizer_t o, const void** out_bytes, size_t* out_size);
int         tcnn_optimizer_deserialize(tcnn_optimizer_t o, const void* bytes, size_t size);
/* Test hook: the Adam kernels take their square root and their division through exact fast forms between range tests, and through sqrtf
 * and `/` outside them.  This runs those very functions against the plain expressions on the device, compares bit for bit, stores nothing
 * per element and waits for the result.  *mismatches: how many inputs differ (expected: 0); *first_bad: the smallest of them, ~0 if none.
 *   TCNN_ADAM_SWEEP_SQRT       every float bit pattern in [first, first + count); first_bad is the pattern
 *   TCNN_ADAM_SWEEP_DIV_GRID   every denominator pattern in [first, first + count) against n_numerators positive numerators whose patterns
 *                              step evenly from numerator_lo to numerator_hi, low 16 bits hashed with seed; first_bad is denominator << 32 | numerator.
 *                              (A denominator outside the division's range test selects the plain expression for every numerator, which
 *                              cannot differ from itself: it is visited with the first numerator only.)
 *   TCNN_ADAM_SWEEP_DIV_PAIRS  `count` pairs drawn from seed around both range tests' edges, a quarter of each operand negative */
#define TCNN_ADAM_SWEEP_SQRT 0
#define TCNN_ADAM_SWEEP_DIV_GRID 1
#define TCNN_ADAM_SWEEP_DIV_PAIRS 2
int         tcnn_adam_math_sweep(tcnn_stream_t stream, int what, uint64_t first, uint64_t count, uint32_t n_numerators, float numerator_lo, float numerator_hi, uint64_t seed,
                                 uint64_t* mismatches, uint64_t* first_bad);


/* ---- standalone losses (loss.h:41-60, src/loss.cu:57-65): the losses a trainer evaluates -- L2, RelativeL2, RelativeL2Luminance, L1,
 * RelativeL1, Mape, Smape, CrossEntropy, Variance -- on predictions the caller owns (a renderer's output, a slice of a module's padded
 * output).  Stateless: a loss is its type number, there is no handle.
 * tcnn_loss_type: the type of a loss configuration ({"otype": ...}, matched case-insensitively; "Invalid loss type: X" otherwise).
 * tcnn_loss_name: the canonical name of a type, or NULL + tcnn_last_error().
 * tcnn_loss_evaluate: Loss<T>::evaluate on `stream`.  prediction: n rows of `dims` values in `precision` (TCNN_PRECISION_FP16 / _FP32), row
 * stride prediction_stride >= dims, unit column stride.  target and data_pdf (or NULL): compact float [n][dims].  Every element is computed
 * by the device code a trainer's loss runs, so values and gradients are bit for bit what a trainer computes from the same predictions.
 * Each output is optional (NULL) and at least one must be given:
 *   values     float [n][values_stride]: the per-element loss, already divided by n * dims;
 *   gradients  [n][gradients_stride] in the prediction's precision: loss_scale * dL/dprediction -- the layout external_dL_dy takes;
 *   loss_sum   one device float: the sum of all values (what tcnn_trainer_loss returns), reduced in a fixed order without storing them:
 *              the same arguments -- the pointers' 16-byte alignment included: it decides between the 16-byte and the element-wise
 *              form, which sum in different orders -- give the same bits, and no floating-point atomics are involved.
 * Columns >= dims of every output row are written as zeros.  scale_dev (or NULL): one device float multiplied into loss_scale in fp32 before
 * the gradient is rounded once to its precision -- an incoming gradient or a gradient scaler's factor, never read by the host.
 * Extents: of the prediction only the n rows of dims values have to be readable, (n - 1) * prediction_stride + dims elements from the
 * pointer -- a column or row slice of a larger matrix is fine; a load never leaves the 16-byte aligned block that holds a value.  target and
 * data_pdf: n * dims floats.  Every requested output is written in full, padding included: n * its stride elements.
 * n is any number of rows (no granularity); n == 0 succeeds, launches nothing and sets *loss_sum to 0.  n * stride must stay below 2^32 for
 * every stride, RelativeL2Luminance needs dims >= 3 (it reads three channels of every row; six when dims >= 6).  All arguments are checked
 * before anything is launched.  The call never synchronises; its workspace comes from the library's stream-ordered arena. */
int         tcnn_loss_type(const char* loss_json, int* type_out);   /* src/loss.cu:57-65 */
const char* tcnn_loss_name(int type);
int         tcnn_loss_evaluate(int type, tcnn_stream_t stream, float loss_scale, const float* scale_dev /* or NULL */,
                               uint32_t n, uint32_t dims, const void* prediction, uint32_t prediction_stride, int precision,
                               const float* target, const float* data_pdf /* or NULL */,
                               float* values, uint32_t values_stride,          /* or NULL */
                               void* gradients, uint32_t gradients_stride,     /* or NULL */
                               float* loss_sum /* device, or NULL */);         /* loss.h:41-49 */

#ifdef __cplusplus
}
#endif
#endif /* TCNN_AMD_H */
