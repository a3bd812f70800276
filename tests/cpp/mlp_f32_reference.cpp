// mlp_f32_reference.cpp -- the numerical contract of the full-precision layer kernels (tiny-cuda-nn_amd/csrc/k_mlp_layers.hip, LayerElem<float>)
// restated on the CPU with std::fmaf: every element of a layer product is one fp32 accumulator that starts at +0 and receives its
// products in ascending k, one fmaf each.  tests/test_fp32_network.py compiles this file with g++ (-ffp-contract=off) and compares the
// GPU's results with what it writes, bit for bit.
//
//   mlp_f32_reference <dir>
// reads   <dir>/spec.txt   "n in_width width n_hidden out_width activation"   (out_width: padded; activation: 0 None, 1 ReLU, of the
//                          hidden layers; the output layer has none)
//         <dir>/x.bin      float [n][in_width]          the network's input
//         <dir>/w.bin      float                        the parameter vector: per layer [rows][cols], input layer first
//         <dir>/dy.bin     float [n][out_width]         dL/doutput
//         <dir>/v.bin      float [n][in_width]          dL/d(dL/dinput), the direction of the second-order pass
// writes  z_<l>.bin, h_<l>.bin   float [n][rows_l]      pre-activation and output of layer l = 0 .. n_hidden
//         g_<l>.bin              float [n][cols_l]      the first-order gradient with respect to layer l's input (g_0 = dL/dinput), through
//                                                       the derivative of the activation below it, as Network::backward computes it
//         d_<l>.bin              float [n][rows_l]      the same from the second-order pass's own first-order pass (a' from its own forward pass)
//         u_<l>.bin              float [n][rows_l]      the tangents u_l = a'(z_l) W_l u_{l-1}, u_{-1} = v (u of the last layer = dL/d(dL/doutput))
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

std::vector<float> read_floats(const std::string& path, size_t count) {
	std::vector<float> v(count);
	FILE* f = std::fopen(path.c_str(), "rb");
	if (!f || std::fread(v.data(), sizeof(float), count, f) != count) {
		std::fprintf(stderr, "cannot read %zu floats from %s\n", count, path.c_str());
		std::exit(2);
	}
	std::fclose(f);
	return v;
}

void write_floats(const std::string& path, const std::vector<float>& v) {
	FILE* f = std::fopen(path.c_str(), "wb");
	if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) {
		std::fprintf(stderr, "cannot write %s\n", path.c_str());
		std::exit(2);
	}
	std::fclose(f);
}

// out[s][r] = sum_k a[s][k] b[r][k], k ascending, one fmaf per product, from +0.  (a: [n][K], b: [R][K])
std::vector<float> product_nt(size_t n, size_t R, size_t K, const float* a, const float* b) {
	std::vector<float> out(n * R);
	for (size_t s = 0; s < n; ++s)
		for (size_t r = 0; r < R; ++r) {
			float acc = 0.0f;
			for (size_t k = 0; k < K; ++k) acc = std::fmaf(b[r * K + k], a[s * K + k], acc);
			out[s * R + r] = acc;
		}
	return out;
}

std::vector<float> transpose(size_t rows, size_t cols, const float* w) {
	std::vector<float> t(rows * cols);
	for (size_t r = 0; r < rows; ++r)
		for (size_t c = 0; c < cols; ++c) t[c * rows + r] = w[r * cols + c];
	return t;
}

} // namespace

int main(int argc, char** argv) {
	if (argc != 2) {
		std::fprintf(stderr, "usage: %s <dir>\n", argv[0]);
		return 2;
	}
	const std::string dir = std::string{argv[1]} + "/";
	unsigned n = 0, in_w = 0, width = 0, n_hidden = 0, out_w = 0, act = 0;
	{
		FILE* f = std::fopen((dir + "spec.txt").c_str(), "r");
		if (!f || std::fscanf(f, "%u %u %u %u %u %u", &n, &in_w, &width, &n_hidden, &out_w, &act) != 6 || act > 1) {
			std::fprintf(stderr, "bad spec.txt\n");
			return 2;
		}
		std::fclose(f);
	}
	const unsigned K = n_hidden + 1;
	std::vector<size_t> rows(K), cols(K), off(K);
	size_t n_params = 0;
	for (unsigned l = 0; l < K; ++l) {
		rows[l] = l == K - 1 ? out_w : width;
		cols[l] = l == 0 ? in_w : width;
		off[l] = n_params;
		n_params += rows[l] * cols[l];
	}
	const std::vector<float> x = read_floats(dir + "x.bin", (size_t)n * in_w), w = read_floats(dir + "w.bin", n_params);
	const std::vector<float> dy = read_floats(dir + "dy.bin", (size_t)n * out_w), v = read_floats(dir + "v.bin", (size_t)n * in_w);
	auto layer_act = [&](unsigned l) { return l == K - 1 ? 0u : act; };

	// forward: h_l = a(z_l), z_l = h_{l-1} W_l^T
	std::vector<std::vector<float>> z(K), h(K);
	for (unsigned l = 0; l < K; ++l) {
		const std::vector<float>& in = l == 0 ? x : h[l - 1];
		z[l] = product_nt(n, rows[l], cols[l], in.data(), w.data() + off[l]);
		h[l] = z[l];
		if (layer_act(l) == 1) for (float& e : h[l]) e = e > 0.0f ? e : 0.0f;
		write_floats(dir + "z_" + std::to_string(l) + ".bin", z[l]);
		write_floats(dir + "h_" + std::to_string(l) + ".bin", h[l]);
	}

	// backward data, twice: as Network::backward multiplies by the derivative (ReLU: the gradient itself, or the gradient times zero), and
	// as the second-order pass does (a' = 1 or 0 from its own forward pass, times the sum)
	for (int second = 0; second < 2; ++second) {
		std::vector<float> d = dy; // with respect to layer l's pre-activation
		if (second) write_floats(dir + "d_" + std::to_string(K - 1) + ".bin", d);
		for (unsigned l = K; l-- > 0;) {
			const std::vector<float> wt = transpose(rows[l], cols[l], w.data() + off[l]);
			std::vector<float> g = product_nt(n, cols[l], rows[l], d.data(), wt.data());
			if (l > 0 && layer_act(l - 1) == 1) {
				for (size_t i = 0; i < g.size(); ++i) {
					const float f = h[l - 1][i];
					g[i] = second ? (f > 0.0f ? 1.0f : 0.0f) * g[i] : (f > 0.0f ? g[i] : g[i] * 0.0f);
				}
			} else if (second) {
				for (float& e : g) e = 1.0f * e;
			}
			if (!second) write_floats(dir + "g_" + std::to_string(l) + ".bin", g);
			else if (l > 0) write_floats(dir + "d_" + std::to_string(l - 1) + ".bin", g);
			d.swap(g);
		}
	}

	// tangents
	std::vector<float> u = v;
	for (unsigned l = 0; l < K; ++l) {
		std::vector<float> next = product_nt(n, rows[l], cols[l], u.data(), w.data() + off[l]);
		for (size_t i = 0; i < next.size(); ++i) next[i] = (layer_act(l) == 1 ? (h[l][i] > 0.0f ? 1.0f : 0.0f) : 1.0f) * next[i];
		write_floats(dir + "u_" + std::to_string(l) + ".bin", next);
		u.swap(next);
	}
	return 0;
}
