// input_jacobian_plan_table.cpp -- which route mlp_input_jacobian_plan chooses for input_jacobian, with its NB and grid, for every
// combination of network, batch size and number of dims listed below: input_gradient_plan_table.cpp's axes (and 2^20 rows, where one class of the rule begins) x n_dims.  Host code only: the
// library loads without a device, Network's constructor touches none.
//
// One line per case:  <otype> <precision> w<width> h<hidden> <activation> n<batch> k<n_dims> layerwise_env<0|1> -> <answer>
// where <answer> is "invalid" (the constructor refuses the configuration), "two-pass", or "fused <name> nb<NB> grid<workgroups>".
// TCNN_AMD_MLP_LAYERWISE is set by this program for each half of the table (Network reads the process switches when it is made).
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>

using namespace tcnn_amd;

static const char* OTYPES[] = {"FullyFusedMLP", "CutlassMLP"};
static const uint32_t WIDTHS[] = {16, 32, 48, 64, 128, 256};
static const uint32_t HIDDEN[] = {0, 1, 2, 3, 4, 5, 6};
static const char* ACTIVATIONS[] = {"None", "ReLU", "LeakyReLU", "Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh"};
static const uint32_t BATCHES[] = {256, 768, 1u << 18, 1u << 20};
static const uint32_t N_DIMS[] = {1, 3, 16, 17};

int main() {
	size_t cases = 0;
	for (int layerwise_env = 0; layerwise_env < 2; ++layerwise_env) {
		if (layerwise_env) setenv("TCNN_AMD_MLP_LAYERWISE", "1", 1);
		else unsetenv("TCNN_AMD_MLP_LAYERWISE");
		switches_reload(); // the process switches, from this environment (as tcnn_create_network does)
		for (const char* otype : OTYPES) for (int fp32 = 0; fp32 < 2; ++fp32) for (uint32_t w : WIDTHS) for (uint32_t h : HIDDEN) for (const char* act : ACTIVATIONS) {
			Json net = Json::object();
			net["otype"] = otype;
			net["n_input_dims"] = 16u;
			net["n_output_dims"] = 17u; // 32 padded columns: every n_dims of the table is a legal call
			net["n_neurons"] = w;
			net["n_hidden_layers"] = h;
			net["activation"] = act;
			net["output_activation"] = "None";
			for (uint32_t n : BATCHES) for (uint32_t k : N_DIMS) {
				++cases;
				printf("%s %s w%u h%u %s n%u k%u layerwise_env%d -> ", otype, fp32 ? "fp32" : "fp16", w, h, act, n, k, layerwise_env);
				try {
					const Network network{net, fp32 ? Precision::Fp32 : Precision::Fp16};
					const MlpInputGradPlan p = network.input_jacobian_plan(n, k);
					if (p.fused) printf("fused %s nb%u grid%u\n", p.name, p.nb, p.grid);
					else printf("%s\n", p.name);
				} catch (const std::exception&) {
					printf("invalid\n");
				}
			}
		}
	}
	printf("%zu cases\n", cases);
	return 0;
}
