// input_gradient_plan_table.cpp -- which route mlp_input_gradient_plan chooses for input_gradient, with its NB and grid, for every
// combination of network and batch size listed below.  Host code only: the library loads without a device, Network's constructor touches none.
//
// One line per case:  <otype> <precision> w<width> h<hidden> <activation> n<batch> layerwise_env<0|1> -> <answer>
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
static const uint32_t BATCHES[] = {256, 768, 1u << 18};

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
			net["n_output_dims"] = 3u;
			net["n_neurons"] = w;
			net["n_hidden_layers"] = h;
			net["activation"] = act;
			net["output_activation"] = "None";
			for (uint32_t n : BATCHES) {
				++cases;
				printf("%s %s w%u h%u %s n%u layerwise_env%d -> ", otype, fp32 ? "fp32" : "fp16", w, h, act, n, layerwise_env);
				try {
					const Network network{net, fp32 ? Precision::Fp32 : Precision::Fp16};
					const MlpInputGradPlan p = network.input_gradient_plan(n);
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
