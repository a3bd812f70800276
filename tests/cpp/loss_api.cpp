// The header API's tcnn::Loss<T>::evaluate (include/tiny-cuda-nn/tcnn_api.h; loss.h:41-60 of the reference) as a caller with its own
// matrices uses it: Smape on half predictions and RelativeL2 on float predictions at n = 256, dims = 3, stride = 16, compared with the
// same float expressions evaluated on the host; the shape checks; the loss_sum overload.  `--no-gpu`: the host-side checks only.
#include <tiny-cuda-nn/loss.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define REQUIRE(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

using tcnn::json;

// float -> binary16 bits, round to nearest even (normal and zero values only: all this test uses)
static uint16_t to_half_bits(float f) {
	uint32_t u;
	std::memcpy(&u, &f, 4);
	const uint32_t sign = (u >> 16) & 0x8000u;
	if ((u & 0x7fffffffu) == 0) return (uint16_t)sign;
	const int32_t e = (int32_t)((u >> 23) & 0xffu) - 127 + 15;
	if (e <= 0 || e >= 31) std::abort();
	uint32_t m = u & 0x7fffffu;
	uint32_t h = ((uint32_t)e << 10) | (m >> 13);
	const uint32_t rest = m & 0x1fffu;
	if (rest > 0x1000u || (rest == 0x1000u && (h & 1u))) ++h;
	return (uint16_t)(sign | h);
}

template <typename F>
static bool throws_with(F&& f, const char* needle) {
	try { f(); } catch (const std::exception& e) { return std::strstr(e.what(), needle) != nullptr; }
	return false;
}

template <typename T>
static void upload(const tcnn::GPUMatrix<T>& m, const std::vector<T>& host) {
	if (host.size() != m.n_elements()) std::abort();
	tcnn::detail::check(tcnn_gpu_memcpy(m.data(), host.data(), m.n_bytes(), TCNN_MEMCPY_HOST_TO_DEVICE));
}

static uint32_t float_bits(float f) {
	uint32_t u;
	std::memcpy(&u, &f, 4);
	return u;
}

// any order of float additions of N values is within (N - 1) 2^-24 sum|v| of their exact sum
static bool sum_within_bound(float sum, const std::vector<float>& values) {
	double exact = 0, magnitude = 0;
	for (float v : values) { exact += v; magnitude += std::fabs(v); }
	return std::fabs((double)sum - exact) <= (double)(values.size() - 1) * std::ldexp(1.0, -24) * magnitude;
}

int main(int argc, char** argv) {
	const bool gpu = !(argc > 1 && std::string{argv[1]} == "--no-gpu");
	const uint32_t n = 256, dims = 3, stride = 16;

	// ---- host: configuration as before; the shape checks of evaluate() come before anything touches a device (no memory behind these)
	{
		for (const char* name : {"L2", "RelativeL2", "RelativeL2Luminance", "L1", "RelativeL1", "Mape", "Smape", "CrossEntropy", "Variance", "smape"}) {
			std::unique_ptr<tcnn::Loss<tcnn::half>> loss{tcnn::create_loss<tcnn::half>({{"otype", name}})};
			REQUIRE(loss->hyperparams().value("otype", "") == name);
			loss->update_hyperparams(json{{"otype", "L1"}}); // a no-op, as in every loss of the reference
			REQUIRE(loss->hyperparams().value("otype", "") == name);
		}
		REQUIRE(throws_with([] { tcnn::Loss<float> bad{json{{"otype", "Huber"}}}; }, "Invalid loss type: Huber"));

		tcnn::Loss<tcnn::half> loss{json{{"otype", "Smape"}}};
		tcnn::half* nowhere = nullptr;
		float* nowhere_f = nullptr;
		tcnn::GPUMatrix<tcnn::half> prediction{nowhere, stride, n}, gradients{nowhere, stride, n}, narrow_gradients{nowhere, dims, n};
		tcnn::GPUMatrix<float> target{nowhere_f, dims, n}, short_target{nowhere_f, dims, n - 1}, values{nowhere_f, stride, n}, narrow_values{nowhere_f, dims, n}, pdf{nowhere_f, dims, n},
			wide_pdf{nowhere_f, stride, n};
		float* sum = nullptr;
		REQUIRE(throws_with([&] { loss.evaluate(1.0f, prediction, short_target, values, gradients); }, "prediction.n() == target.n()"));
		REQUIRE(throws_with([&] { loss.evaluate(1.0f, prediction, target, narrow_values, gradients); }, "values.m() == stride"));
		REQUIRE(throws_with([&] { loss.evaluate(nullptr, 1.0f, prediction, target, values, narrow_gradients); }, "gradients.m() == stride"));
		REQUIRE(throws_with([&] { loss.evaluate(nullptr, 1.0f, prediction, target, values, gradients, &wide_pdf); }, "data_pdf->m() == dims"));
		REQUIRE(throws_with([&] { loss.evaluate(nullptr, 1.0f, prediction, short_target, sum, gradients); }, "prediction.n() == target.n()"));
		REQUIRE(throws_with([&] { loss.evaluate(nullptr, 1.0f, prediction, target, sum, narrow_gradients); }, "gradients.m() == stride"));
		REQUIRE(throws_with([&] { loss.evaluate(nullptr, 1.0f, prediction, target, sum, gradients, &wide_pdf); }, "data_pdf->m() == dims"));
		REQUIRE(throws_with([&] { loss.evaluate(nullptr, 1.0f, prediction, target, sum, gradients, &pdf); }, "loss_sum != nullptr"));
		// the library's own checks arrive as its message: all shapes right, but no memory behind any output
		REQUIRE(throws_with([&] { loss.evaluate(nullptr, 1.0f, prediction, target, values, gradients, &pdf); }, "tcnn_loss_evaluate: no output requested"));
	}
	std::printf("host checks ok\n");
	if (!gpu) return 0;

	// ---- device.  Predictions are multiples of 1/64 in [1/16, 2]: exact in half.  Padding columns hold a value no result contains.
	std::vector<float> p((size_t)n * stride, 3.0f), t((size_t)n * dims), q((size_t)n * dims);
	uint32_t state = 12345u;
	const auto next = [&] { state = state * 1664525u + 1013904223u; return state >> 8; };
	for (uint32_t i = 0; i < n; ++i) {
		for (uint32_t j = 0; j < dims; ++j) {
			p[(size_t)i * stride + j] = (float)(4 + next() % 125) / 64.0f;
			t[(size_t)i * dims + j] = 0.05f + 1.95f * (float)(next() % 4096) / 4096.0f;
			q[(size_t)i * dims + j] = 0.5f + 1.5f * (float)(next() % 4096) / 4096.0f;
		}
	}
	tcnn::GPUMatrix<float> target{dims, n}, pdf{dims, n}, values{stride, n};
	upload(target, t);
	upload(pdf, q);
	const float n_total = (float)(n * dims);

	{ // Loss<half>, Smape (smape.h:40-73), loss scale 128
		const float loss_scale = 128.0f;
		std::vector<tcnn::half> ph(p.size());
		for (size_t i = 0; i < p.size(); ++i) ph[i].bits = to_half_bits(p[i]);
		tcnn::GPUMatrix<tcnn::half> prediction{stride, n}, gradients{stride, n}, gradients2{stride, n};
		upload(prediction, ph);
		values.memset(0xff);
		gradients.memset(0xff);
		std::unique_ptr<tcnn::Loss<tcnn::half>> loss{tcnn::create_loss<tcnn::half>({{"otype", "Smape"}})};
		loss->evaluate(nullptr, loss_scale, prediction, target, values, gradients, &pdf);
		const std::vector<float> v = values.to_cpu_vector();
		const std::vector<tcnn::half> g = gradients.to_cpu_vector();
		std::vector<float> compact;
		for (uint32_t i = 0; i < n; ++i) {
			for (uint32_t j = 0; j < stride; ++j) {
				const size_t at = (size_t)i * stride + j;
				if (j >= dims) {
					REQUIRE(float_bits(v[at]) == 0 && g[at].bits == 0);
					continue;
				}
				const float prediction_ = p[at], target_ = t[(size_t)i * dims + j], pdf_ = q[(size_t)i * dims + j];
				const float difference = prediction_ - target_;
				const float scale = 1.0f / (0.5f * (std::fabs(target_) + std::fabs(prediction_)) + 1e-2f) / pdf_;
				const float value = std::fabs(difference) * scale / n_total;
				const float gradient = std::copysign(scale, difference);
				REQUIRE(float_bits(v[at]) == float_bits(value));
				REQUIRE(g[at].bits == to_half_bits(loss_scale * gradient / n_total));
				compact.push_back(v[at]);
			}
		}
		// the loss_sum overload: the same gradients, and the sum of those values
		tcnn::GPUMemory<float> sum(1);
		gradients2.memset(0xff);
		loss->evaluate(nullptr, loss_scale, prediction, target, sum.data(), gradients2, &pdf);
		const std::vector<tcnn::half> g2 = gradients2.to_cpu_vector();
		REQUIRE(std::memcmp(g.data(), g2.data(), g.size() * sizeof(tcnn::half)) == 0);
		float host_sum = 0;
		sum.copy_to_host(&host_sum);
		REQUIRE(host_sum > 0 && sum_within_bound(host_sum, compact));
	}

	{ // Loss<float>, RelativeL2 (relative_l2.h:60-73), loss scale 1, no pdf, the overload without a stream
		tcnn::GPUMatrix<float> prediction{stride, n}, gradients{stride, n};
		upload(prediction, p);
		values.memset(0xff);
		gradients.memset(0xff);
		tcnn::Loss<float> loss{json{{"otype", "RelativeL2"}}};
		loss.evaluate(1.0f, prediction, target, values, gradients);
		const std::vector<float> v = values.to_cpu_vector(), g = gradients.to_cpu_vector();
		std::vector<float> compact;
		for (uint32_t i = 0; i < n; ++i) {
			for (uint32_t j = 0; j < stride; ++j) {
				const size_t at = (size_t)i * stride + j;
				if (j >= dims) {
					REQUIRE(float_bits(v[at]) == 0 && float_bits(g[at]) == 0);
					continue;
				}
				const float prediction_ = p[at], target_ = t[(size_t)i * dims + j], pdf_ = 1;
				const float difference = prediction_ - target_;
				const float prediction_sq_plus_epsilon = prediction_ * prediction_ + 0.01f;
				const float value = difference * difference / prediction_sq_plus_epsilon / pdf_ / n_total;
				const float gradient = 2 * difference / prediction_sq_plus_epsilon / pdf_;
				REQUIRE(float_bits(v[at]) == float_bits(value));
				REQUIRE(float_bits(g[at]) == float_bits(1.0f * gradient / n_total));
				compact.push_back(v[at]);
			}
		}
		tcnn::GPUMemory<float> sum(1);
		loss.evaluate(nullptr, 1.0f, prediction, target, sum.data(), gradients);
		float host_sum = 0;
		sum.copy_to_host(&host_sum);
		REQUIRE(host_sum > 0 && sum_within_bound(host_sum, compact));
	}
	std::printf("gpu checks ok\n");
	return 0;
}
