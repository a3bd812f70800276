// input_jvp_backward_plan_table.cpp -- which route mlp_input_jvp_backward_plan chooses for input_jvp_backward, with its NB, TT and grid, for
// every combination of network, batch size and number of tangents listed below: input_jvp_plan_table.cpp's axes.  Host code only: the library
// loads without a device, Network's constructor touches none.  Every case is asked twice: the plan is a pure function of its arguments.
// The output is compared with tests/golden/input_jvp_backward_plan_table.txt.
//
// One line per group of networks that differ in the activation alone and get the same answers:
//   <otype> <precision> w<width> h<hidden> <activation>[,<activation>...] layerwise_env<0|1> -> <answers>
// (the first such group of a shape is written "*": every activation that no later line of the shape names)
// where <answers> is "invalid" (the constructor refuses the configuration), "all <answer>" if every batch size and number of tangents gets
// the same answer, else "n<batch> t<n_tangents> <answer>" for each of them, separated by "; ".  An <answer> is "two-pass" or
// "fused <name> nb<NB> tt<TT> grid<workgroups>".
// TCNN_AMD_MLP_LAYERWISE is set by this program for each half of the table (Network reads the process switches when it is made).
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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
		for (const char* otype : OTYPES) for (int fp32 = 0; fp32 < 2; ++fp32) for (uint32_t w : WIDTHS) for (uint32_t h : HIDDEN) {
			std::vector<std::pair<std::string, std::string>> groups; // (activations, answers), in order of first appearance
			for (const char* act : ACTIVATIONS) {
				Json net = Json::object();
				net["otype"] = otype;
				net["n_input_dims"] = 16u;
				net["n_output_dims"] = 17u;
				net["n_neurons"] = w;
				net["n_hidden_layers"] = h;
				net["activation"] = act;
				net["output_activation"] = "None";
				std::vector<std::string> answers, keys;
				bool invalid = false;
				for (uint32_t n : BATCHES) for (uint32_t t : N_TANGENTS) {
					++cases;
					try {
						const Network network{net, fp32 ? Precision::Fp32 : Precision::Fp16};
						const MlpInputJvpBackwardPlan p = network.input_jvp_backward_plan(n, t), again = network.input_jvp_backward_plan(n, t);
						if (p.fused != again.fused || strcmp(p.name, again.name) != 0 || p.nb != again.nb || p.tt != again.tt || p.grid != again.grid || p.relu != again.relu) {
							printf("not a pure function\n");
							return 1;
						}
						char text[128];
						if (p.fused) snprintf(text, sizeof(text), "fused %s nb%u tt%u grid%u", p.name, p.nb, p.tt, p.grid);
						else snprintf(text, sizeof(text), "%s", p.name);
						answers.push_back(text);
						keys.push_back("n" + std::to_string(n) + " t" + std::to_string(t));
					} catch (const std::exception&) {
						invalid = true;
					}
				}
				std::string line;
				bool same = true;
				for (const std::string& a : answers) same = same && a == answers[0];
				if (invalid) line = "invalid";
				else if (same) line = "all " + answers[0];
				else for (size_t i = 0; i < answers.size(); ++i) line += (i ? "; " : "") + keys[i] + " " + answers[i];
				bool found = false;
				for (auto& g : groups) {
					if (g.second == line) {
						g.first += std::string{","} + act;
						found = true;
						break;
					}
				}
				if (!found) groups.emplace_back(act, line);
			}
			// (the first group is written "*" where the others name their activations: "every activation not named on another line of this network shape")
			for (size_t i = 0; i < groups.size(); ++i) {
				printf("%s %s w%u h%u %s layerwise_env%d -> %s\n", otype, fp32 ? "fp32" : "fp16", w, h, i ? groups[i].first.c_str() : "*", layerwise_env, groups[i].second.c_str());
			}
		}
	}
	printf("%zu cases\n", cases);
	return 0;
}
