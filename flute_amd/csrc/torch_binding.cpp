// Compiled torch-dispatcher binding of the C ABI: `flute::qgemm_raw_simple[_hadamard]`.
//
// Role of flute/csrc/qgemm.cpp:86-198 (qgemm_raw_simple), :214-244 (qgemm_raw_simple_hadamard) and the
// registrations :246-260: same schemas (verbatim), implemented for dispatch key CUDA (HIP tensors use it on
// PyTorch-ROCm).  The function body is host glue only - validate, flatten input[..., K] -> [M, K], allocate
// D[M, N], device guard, current stream - and ONE call into libflute_amd.so (include/flute_amd.h); no device
// code lives here (plain C++ translation unit).  Round 1 did this glue in Python + ctypes: 18.9 us per eager
// call against a 6 us kernel.
#include <ATen/ATen.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <cstdint>

#include "../../include/flute_amd.h"

namespace {

int dtype_id(const at::Tensor& t) {
    if (t.scalar_type() == at::kHalf) return FLUTE_F16;
    if (t.scalar_type() == at::kBFloat16) return FLUTE_BF16;
    TORCH_CHECK_TYPE(false, "Only fp16 and bf16 supported currently");
    return -1;
}

// A tensor as the C ABI takes it (include/flute_amd.h: contiguous, 16-B aligned): borrowed when it already is - no
// allocation, no operator call - otherwise a fresh contiguous copy, which the allocator aligns.  A contiguous view such
// as buf[1:1 + n] is not aligned, and the kernels address their operands with 16-B loads and buffer descriptors.
c10::MaybeOwned<at::Tensor> abi_tensor(const at::Tensor& t) {
    if (t.is_contiguous() && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0)
        return c10::MaybeOwned<at::Tensor>::borrowed(t);
    return c10::MaybeOwned<at::Tensor>::owned(t.clone(at::MemoryFormat::Contiguous));
}

// flute/ops.py:17-49 (the reference validates in its fake impl only and trusts raw pointers in the real one,
// qgemm.cpp:71-77; here both validate)
void validate(const at::Tensor& input, const at::Tensor& weight, const at::Tensor& scales, const at::Tensor& table,
              const at::Tensor& table2, const at::Tensor& workspace, int64_t num_bits, int64_t group_size) {
    TORCH_CHECK_VALUE(input.dim() >= 2 && weight.dim() == 2 && scales.dim() == 2 && table.dim() == 1 &&
                          table2.dim() == 3 && workspace.dim() == 1,
                      "flute::qgemm_raw_simple: wrong tensor ranks");
    const auto dt = input.scalar_type();
    TORCH_CHECK_TYPE(dt == at::kHalf || dt == at::kBFloat16, "Only fp16 and bf16 supported currently");
    TORCH_CHECK_TYPE(weight.scalar_type() == at::kShort && scales.scalar_type() == dt && table.scalar_type() == dt &&
                         table2.scalar_type() == at::kFloat && workspace.scalar_type() == at::kByte,
                     "flute::qgemm_raw_simple: wrong dtypes");
    TORCH_CHECK_VALUE(num_bits >= 1 && num_bits <= 8, "Unsupported num_bits value");
    const int64_t K = input.size(-1), N = scales.size(0), L = int64_t(1) << num_bits;
    TORCH_CHECK_VALUE(weight.size(1) == K && K == scales.size(1) * group_size &&
                          weight.size(0) == (int64_t)(num_bits * (N / 16.0)) && table.size(0) == L &&
                          table2.size(0) == L && table2.size(1) == L && table2.size(2) == 1,
                      "flute::qgemm_raw_simple: inconsistent shapes");
}

at::Tensor qgemm_impl(const at::Tensor& input, const at::Tensor& weight, const at::Tensor& scales,
                      const at::Tensor& table, const at::Tensor& table2, at::Tensor& workspace, int64_t num_bits,
                      int64_t group_size, int64_t hadamard_size, int64_t template_id, int64_t num_sms) {
    validate(input, weight, scales, table, table2, workspace, num_bits, group_size);
    TORCH_CHECK(weight.is_contiguous() && scales.is_contiguous() && table.is_contiguous() && table2.is_contiguous() &&
                    workspace.is_contiguous(),
                "flute::qgemm_raw_simple: weight/scales/tables/workspace must be contiguous");
    const auto dev = input.device();
    TORCH_CHECK(weight.device() == dev && scales.device() == dev && table.device() == dev && table2.device() == dev &&
                    workspace.device() == dev,
                "flute::qgemm_raw_simple: all tensors must be on the input's device");
    const int64_t K = input.size(-1), N = scales.size(0);
    const bool flat = input.dim() == 2 && input.is_contiguous();          // the decode-loop case: no view objects at all
    at::Tensor reshaped;
    if (!flat) reshaped = input.reshape({-1, K});
    const c10::MaybeOwned<at::Tensor> x2d_ = abi_tensor(*(flat ? &input : &reshaped));
    const c10::MaybeOwned<at::Tensor> weight_ = abi_tensor(weight), scales_ = abi_tensor(scales),
                                      table_ = abi_tensor(table), table2_ = abi_tensor(table2);
    const at::Tensor& x2d = *x2d_;
    const int64_t M = x2d.size(0);
    at::Tensor out = at::empty({M, N}, input.options());
    if (M > 0) {
        const int dt = dtype_id(input);
        if (hadamard_size != 0) {
            if (hadamard_size < 1 || (hadamard_size & (hadamard_size - 1)) || hadamard_size > (1 << 15))
                TORCH_CHECK(false, flute_strerror(FLUTE_ERR_HADAMARD_SIZE));
            TORCH_CHECK(K % hadamard_size == 0 || (M * K) % hadamard_size == 0, "shape is invalid for hadamard_size ",
                        hadamard_size);
        }
        // PyTorch-ROCm keeps DeviceType::CUDA for HIP devices: the "masquerading" guard / stream types
        const c10::hip::HIPGuardMasqueradingAsCUDA guard(dev);                // qgemm.cpp:101 OptionalCUDAGuard
        at::Tensor scratch;
        void* scratch_ptr = nullptr;
        // decode-kernel launches rotate the activations while staging them; every other plan rotates into a
        // scratch tensor first (qgemm.cpp:201-244)
        if (hadamard_size > 1 && !flute_qgemm_hadamard_fused(dt, (int)num_bits, (int)group_size, (int)hadamard_size,
                                                             (int)M, (int)N, (int)K, (int)template_id, (int)num_sms,
                                                             (size_t)workspace.numel())) {
            scratch = at::empty_like(x2d);
            scratch_ptr = scratch.data_ptr();
        }
        const hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dev.index()).stream();   // qgemm.cpp:105
        const int rc = flute_qgemm_hadamard(dt, (int)num_bits, (int)group_size, (int)hadamard_size, (int)M, (int)N,
                                            (int)K, (int)weight.size(0), x2d.data_ptr(), weight_->data_ptr(),
                                            out.data_ptr(), scales_->data_ptr(), table_->data_ptr(), table2_->data_ptr(),
                                            scratch_ptr, workspace.data_ptr(), (size_t)workspace.numel(),
                                            (int)template_id, (int)num_sms, stream);
        TORCH_CHECK(rc == FLUTE_OK, flute_strerror(rc));      // RuntimeError with the reference's message prefixes
    }
    if (flat) return out;
    auto shape = input.sizes().vec();
    shape.back() = N;
    return out.reshape(shape);
}

at::Tensor qgemm_raw_simple(const at::Tensor& input, const at::Tensor& weight, const at::Tensor& scales,
                            const at::Tensor& table, const at::Tensor& table2, at::Tensor& workspace,
                            int64_t num_bits, int64_t group_size, int64_t template_id, int64_t num_sms) {
    return qgemm_impl(input, weight, scales, table, table2, workspace, num_bits, group_size, 0, template_id, num_sms);
}

at::Tensor qgemm_raw_simple_hadamard(const at::Tensor& input, const at::Tensor& weight, const at::Tensor& scales,
                                     const at::Tensor& table, const at::Tensor& table2, at::Tensor& workspace,
                                     int64_t num_bits, int64_t group_size, int64_t hadamard_size,
                                     int64_t template_id, int64_t num_sms) {
    return qgemm_impl(input, weight, scales, table, table2, workspace, num_bits, group_size, hadamard_size,
                      template_id, num_sms);
}

// ---- flute_amd::dequantize: the dense weight [N, K] (flute_dequantize) ----------------------------------------------

// the shapes / dtypes / devices of (weight, scales, table2) as one layer; returns N
int64_t check_dequant_args(const at::Tensor& weight, const at::Tensor& scales, const at::Tensor& table2,
                           int64_t num_bits, int64_t group_size) {
    TORCH_CHECK_VALUE(weight.dim() == 2 && scales.dim() == 2 && table2.dim() == 3,
                      "flute_amd::dequantize: wrong tensor ranks");
    const auto dt = scales.scalar_type();
    TORCH_CHECK_TYPE(dt == at::kHalf || dt == at::kBFloat16, "Only fp16 and bf16 supported currently");
    TORCH_CHECK_TYPE(weight.scalar_type() == at::kShort && table2.scalar_type() == at::kFloat,
                     "flute_amd::dequantize: wrong dtypes");
    TORCH_CHECK_VALUE(num_bits >= 1 && num_bits <= 8, "Unsupported num_bits value");
    const int64_t K = weight.size(1), N = scales.size(0), L = int64_t(1) << num_bits;
    TORCH_CHECK_VALUE(K == scales.size(1) * group_size && weight.size(0) == (int64_t)(num_bits * (N / 16.0)) &&
                          table2.size(0) == L && table2.size(1) == L && table2.size(2) == 1,
                      "flute_amd::dequantize: inconsistent shapes");
    TORCH_CHECK(weight.is_contiguous() && scales.is_contiguous() && table2.is_contiguous(),
                "flute_amd::dequantize: weight/scales/table2 must be contiguous");
    TORCH_CHECK(weight.device() == scales.device() && table2.device() == scales.device(),
                "flute_amd::dequantize: all tensors must be on the same device");
    return N;
}

// columns [k0, k0 + W.size(1)) of the dense weight into W ([N, k_count] contiguous, scales' dtype); weight, scales and table2
// as abi_tensor returns them (the callers realign once, not per chunk)
void dequantize_into(const at::Tensor& weight, const at::Tensor& scales, const at::Tensor& table2, int64_t num_bits,
                     int64_t group_size, int64_t template_id, int64_t k0, at::Tensor& W) {
    const c10::hip::HIPGuardMasqueradingAsCUDA guard(scales.device());
    const hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(scales.device().index()).stream();
    const int rc = flute_dequantize(dtype_id(scales), (int)num_bits, (int)group_size, (int)scales.size(0),
                                    (int)weight.size(1), (int)weight.size(0), (int)k0, (int)W.size(1),
                                    weight.data_ptr(), scales.data_ptr(), table2.data_ptr(), W.data_ptr(),
                                    (int)template_id, stream);
    TORCH_CHECK(rc == FLUTE_OK, flute_strerror(rc));
}

at::Tensor dequantize(const at::Tensor& weight, const at::Tensor& scales, const at::Tensor& table2, int64_t num_bits,
                      int64_t group_size, int64_t template_id) {
    const int64_t N = check_dequant_args(weight, scales, table2, num_bits, group_size);
    at::Tensor W = at::empty({N, weight.size(1)}, scales.options());
    dequantize_into(*abi_tensor(weight), *abi_tensor(scales), *abi_tensor(table2), num_bits, group_size, template_id, 0, W);
    return W;
}

// ---- autograd kernels of flute::qgemm_raw_simple[_hadamard] --------------------------------------------------------
// The input gradient only: dX = dY @ W, W = dequantize(Q, S, QM2) [N, K] (then the orthonormal, symmetric Sylvester
// rotation of the _hadamard form: D = had(X) @ W^T, so dX = had(dY @ W)).  The dense weight is built in K-column chunks of at
// most kBackwardScratchBytes, each multiplied at once by hipBLASLt (at::mm): every element of dX is still one full-N
// reduction, so the chunking adds no rounding.  No gradient for scales / table / table2: a graph that needs one raises.

constexpr int64_t kBackwardScratchBytes = int64_t(128) << 20;

at::Tensor qgemm_input_grad(const at::Tensor& dY, const at::Tensor& weight, const at::Tensor& scales,
                            const at::Tensor& table2, int64_t num_bits, int64_t group_size, int64_t hadamard_size,
                            int64_t template_id, at::IntArrayRef input_shape) {
    TORCH_CHECK(dY.is_cuda() && scales.is_cuda(), "flute::qgemm_raw_simple: the backward needs GPU tensors");
    const int64_t N = scales.size(0), K = weight.size(1);
    const at::Tensor dy = dY.reshape({-1, N});
    const int64_t M = dy.size(0);
    at::Tensor dx = at::empty({M, K}, dY.options().memory_format(at::MemoryFormat::Contiguous));
    if (M > 0) {
        // a power-of-two chunk width: hipBLASLt ran 2304-wide chunks of 8192 x 28672 at half the speed of 2048-wide ones
        // (M = 4096: 2832 vs 1526 us for the four chunk GEMMs, profiles/dequant/chunk_gemm_shapes.jsonl)
        int64_t kc = 64;
        while (kc * 2 * N * 2 <= kBackwardScratchBytes) kc *= 2;
        at::Tensor W = at::empty({N, std::min(kc, K)}, scales.options());
        const c10::MaybeOwned<at::Tensor> weight_ = abi_tensor(weight), scales_ = abi_tensor(scales), table2_ = abi_tensor(table2);
        for (int64_t k0 = 0; k0 < K; k0 += kc) {
            const int64_t kn = std::min(kc, K - k0);
            at::Tensor Wc = kn == W.size(1) ? W : W.narrow(1, 0, kn).contiguous();
            dequantize_into(*weight_, *scales_, *table2_, num_bits, group_size, template_id, k0, Wc);
            if (kn == K) {
                at::mm_out(dx, dy, Wc);
            } else {
                at::Tensor dxc = dx.narrow(1, k0, kn);
                at::mm_out(dxc, dy, Wc);
            }
        }
        if (hadamard_size > 1) {
            const c10::hip::HIPGuardMasqueradingAsCUDA guard(dx.device());
            const hipStream_t stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(dx.device().index()).stream();
            const int rc = flute_hadamard(dtype_id(dx), dx.data_ptr(), dx.data_ptr(), (size_t)dx.numel(),
                                          (uint32_t)hadamard_size, stream);
            TORCH_CHECK(rc == FLUTE_OK, flute_strerror(rc));
        }
    }
    return dx.view(input_shape);
}

// the kernels below autograd: what the op computes without a graph
at::Tensor qgemm_below_autograd(c10::DispatchKeySet ks, const at::Tensor& input, const at::Tensor& weight,
                                const at::Tensor& scales, const at::Tensor& table, const at::Tensor& table2,
                                at::Tensor& workspace, int64_t num_bits, int64_t group_size, int64_t hadamard_size,
                                int64_t template_id, int64_t num_sms) {
    if (hadamard_size == 0) {
        static auto op = c10::Dispatcher::singleton()
                             .findSchemaOrThrow("flute::qgemm_raw_simple", "")
                             .typed<decltype(qgemm_raw_simple)>();
        return op.redispatch(ks, input, weight, scales, table, table2, workspace, num_bits, group_size, template_id,
                             num_sms);
    }
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("flute::qgemm_raw_simple_hadamard", "")
                         .typed<decltype(qgemm_raw_simple_hadamard)>();
    return op.redispatch(ks, input, weight, scales, table, table2, workspace, num_bits, group_size, hadamard_size,
                         template_id, num_sms);
}

class QGemmFunction : public torch::autograd::Function<QGemmFunction> {
   public:
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& input, const at::Tensor& weight,
                              const at::Tensor& scales, const at::Tensor& table, const at::Tensor& table2,
                              at::Tensor& workspace, int64_t num_bits, int64_t group_size, int64_t hadamard_size,
                              int64_t template_id, int64_t num_sms, c10::DispatchKeySet ks) {
        at::AutoDispatchBelowADInplaceOrView guard;
        at::Tensor out = qgemm_below_autograd(ks, input, weight, scales, table, table2, workspace, num_bits,
                                              group_size, hadamard_size, template_id, num_sms);
        ctx->save_for_backward({weight, scales, table2});
        ctx->saved_data["num_bits"] = num_bits;
        ctx->saved_data["group_size"] = group_size;
        ctx->saved_data["hadamard_size"] = hadamard_size;
        ctx->saved_data["template_id"] = template_id;
        ctx->saved_data["input_shape"] = input.sizes().vec();
        return out;
    }

    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx,
                                                   torch::autograd::variable_list grads) {
        // inputs: input, weight, scales, table, table2, workspace, then the ints and the key set
        TORCH_CHECK(!ctx->needs_input_grad(2) && !ctx->needs_input_grad(3) && !ctx->needs_input_grad(4),
                    "flute::qgemm_raw_simple: gradients with respect to scales, table or table2 are not supported "
                    "(only the input gradient is); detach them or set requires_grad=False");
        const at::Tensor& dY = grads[0];
        TORCH_CHECK(!(at::GradMode::is_enabled() && dY.requires_grad()),
                    "flute::qgemm_raw_simple: the backward is once-differentiable (no double backward)");
        torch::autograd::variable_list out(12);
        if (ctx->needs_input_grad(0) && dY.defined()) {
            const auto saved = ctx->get_saved_variables();
            const auto shape = ctx->saved_data["input_shape"].toIntVector();
            out[0] = qgemm_input_grad(dY, saved[0], saved[1], saved[2], ctx->saved_data["num_bits"].toInt(),
                                      ctx->saved_data["group_size"].toInt(), ctx->saved_data["hadamard_size"].toInt(),
                                      ctx->saved_data["template_id"].toInt(), shape);
        }
        return out;
    }
};

bool any_requires_grad(const at::Tensor& input, const at::Tensor& scales, const at::Tensor& table,
                       const at::Tensor& table2) {
    return at::GradMode::is_enabled() &&
           (input.requires_grad() || scales.requires_grad() || table.requires_grad() || table2.requires_grad());
}

at::Tensor qgemm_raw_simple_autograd(c10::DispatchKeySet ks, const at::Tensor& input, const at::Tensor& weight,
                                     const at::Tensor& scales, const at::Tensor& table, const at::Tensor& table2,
                                     at::Tensor& workspace, int64_t num_bits, int64_t group_size, int64_t template_id,
                                     int64_t num_sms) {
    if (!any_requires_grad(input, scales, table, table2))
        return qgemm_below_autograd(ks & c10::after_autograd_keyset, input, weight, scales, table, table2, workspace,
                                    num_bits, group_size, 0, template_id, num_sms);
    return QGemmFunction::apply(input, weight, scales, table, table2, workspace, num_bits, group_size, int64_t(0),
                                template_id, num_sms, ks & c10::after_ADInplaceOrView_keyset);
}

at::Tensor qgemm_raw_simple_hadamard_autograd(c10::DispatchKeySet ks, const at::Tensor& input,
                                              const at::Tensor& weight, const at::Tensor& scales,
                                              const at::Tensor& table, const at::Tensor& table2,
                                              at::Tensor& workspace, int64_t num_bits, int64_t group_size,
                                              int64_t hadamard_size, int64_t template_id, int64_t num_sms) {
    if (!any_requires_grad(input, scales, table, table2))
        return qgemm_below_autograd(ks & c10::after_autograd_keyset, input, weight, scales, table, table2, workspace,
                                    num_bits, group_size, hadamard_size, template_id, num_sms);
    return QGemmFunction::apply(input, weight, scales, table, table2, workspace, num_bits, group_size, hadamard_size,
                                template_id, num_sms, ks & c10::after_ADInplaceOrView_keyset);
}

}  // namespace

// flute/csrc/qgemm.cpp:251-254, verbatim
TORCH_LIBRARY(flute, m) {
    m.def("qgemm_raw_simple(Tensor input, Tensor weight, Tensor scales, Tensor table, Tensor table2, "
          "Tensor(a!) workspace, int num_bits, int group_size, int template_id, int num_sms) -> Tensor");
    m.def("qgemm_raw_simple_hadamard(Tensor input, Tensor weight, Tensor scales, Tensor table, Tensor table2, "
          "Tensor(a!) workspace, int num_bits, int group_size, int hadamard_size, int template_id, int num_sms) "
          "-> Tensor");
}

// flute/csrc/qgemm.cpp:257-260
TORCH_LIBRARY_IMPL(flute, CUDA, m) {
    m.impl("qgemm_raw_simple", &qgemm_raw_simple);
    m.impl("qgemm_raw_simple_hadamard", &qgemm_raw_simple_hadamard);
}

// Autograd kernels (input gradient only): above.  Without a tensor that requires grad they redispatch at once.
TORCH_LIBRARY_IMPL(flute, Autograd, m) {
    m.impl("qgemm_raw_simple", &qgemm_raw_simple_autograd);
    m.impl("qgemm_raw_simple_hadamard", &qgemm_raw_simple_hadamard_autograd);
}

// This project's own operators (the reference has none of these): flute_amd::dequantize, the dense weight [N, K].
TORCH_LIBRARY(flute_amd, m) {
    m.def("dequantize(Tensor weight, Tensor scales, Tensor table2, int num_bits, int group_size, int template_id) "
          "-> Tensor");
}

TORCH_LIBRARY_IMPL(flute_amd, CUDA, m) { m.impl("dequantize", &dequantize); }
