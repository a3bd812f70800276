// input_jvp_plan_table.cpp -- which route mlp_input_jvp_plan chooses for input_jvp, with its NB, TT and grid, for every combination of
// network, batch size and number of tangents listed below: input_jacobian_plan_table.cpp's axes x n_tangents.  Host code only: the library
// loads without a device, Network's constructor touches none.  Every case is asked twice: the plan is a pure function of its arguments.
//
// One line per case:  <otype> <precision> w<width> h<hidden> <activation> n<batch> t<n_tangents> layerwise_env<0|1> -> <answer>
// where <answer> is "invalid" (the constructor refuses the configuration), "two-pass", or "fused <name> nb<NB> tt<TT> grid<workgroups>".
// TCNN_AMD_MLP_LAYERWISE is set by this program for each half of the table (Network reads the process switches when it is made).
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace tcnn_amd;

static const char* OTYPES[] = {"FullyFusedMLP", "CutlassMLP"};
static const uint32_t WIDTHS[] = {16, 32, 48, 64, 128, 256};
static const uint32_t HIDDEN[] = {0, 1, 2, 3, 4, 5, 6};
static const char* ACTIVATIONS[] = {"None", "ReLU", "LeakyReLU", "Exponential", "Sine", "Sigmoid", "Squareplus", "Softplus", "Tanh"};
static const uint32_t BATCHES[] = {256, 768, 1u << 18, 1u << 20};
static const uint32_t N_TANGENTS[] = {1, 2, 3, 4};

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
			net["n_output_dims"] = 17u;
			net["n_neurons"] = w;
			net["n_hidden_layers"] = h;
			net["activation"] = act;
			net["output_activation"] = "None";
			for (uint32_t n : BATCHES) for (uint32_t t : N_TANGENTS) {
				++cases;
				printf("%s %s w%u h%u %s n%u t%u layerwise_env%d -> ", otype, fp32 ? "fp32" : "fp16", w, h, act, n, t, layerwise_env);
				try {
					const Network network{net, fp32 ? Precision::Fp32 : Precision::Fp16};
					const MlpInputJvpPlan p = network.input_jvp_plan(n, t), again = network.input_jvp_plan(n, t);
					if (p.fused != again.fused || strcmp(p.name, again.name) != 0 || p.nb != again.nb || p.tt != again.tt || p.grid != again.grid || p.relu != again.relu) {
						printf("not a pure function\n");
						return 1;
					}
					if (p.fused) printf("fused %s nb%u tt%u grid%u\n", p.name, p.nb, p.tt, p.grid);
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
