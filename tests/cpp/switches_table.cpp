// switches_table.cpp -- what switches_reload() makes of the environment.  Host code only: the library loads without a device.
//
// Every argument is one environment: "NAME=VALUE", or "-" for the empty one.  Per argument the program removes every TCNN_AMD_* variable,
// sets that one, calls switches_reload() and prints every field of switches() on one line.  The expected lines are in tests/test_switches.py.
#include "../../tiny-cuda-nn_amd/csrc/tcnn_common.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern char** environ;

using namespace tcnn_amd;

static void clear_environment() {
	std::vector<std::string> names;
	for (char** e = environ; *e; ++e)
		if (strncmp(*e, "TCNN_AMD_", 9) == 0) names.emplace_back(*e, strcspn(*e, "="));
	for (const std::string& n : names) unsetenv(n.c_str());
}

int main(int argc, char** argv) {
	for (int i = 1; i < argc; ++i) {
		clear_environment();
		const std::string arg = argv[i];
		const size_t eq = arg.find('=');
		if (arg != "-") {
			if (eq == std::string::npos) return 2;
			setenv(arg.substr(0, eq).c_str(), arg.substr(eq + 1).c_str(), 1);
		}
		switches_reload();
		const Switches w = switches();
		printf("%s: grid_planes=%d grid_rows_planes=%d grid_scatter_lds=%d scatter_records=%d scatter_tune=%d scatter_lists=%d scatter_wide=%d fused_step=%d side_jobs=%d live_image=%d "
		       "adam_steps32=%d adam_in_reduce=%d adam_prologue=%d adam_prologue_refused=%d mlp_r32=%d mlp_r32a=%d mlp_regs=%d mlp_fast=%d mlp_prio=%u listgrad_in_mlp=%d mlp_layerwise=%d "
		       "mlp_regw=%d mlp_variant_forced=%d mlp_variant=%d,%d,%d wgrad_rows=%d mlp_fwd_lds=%d fuse_oneblob=%d\n",
		       arg.c_str(), w.grid_planes, w.grid_rows_planes, w.grid_scatter_lds, w.scatter_records, w.scatter_tune, w.scatter_lists, w.scatter_wide, w.fused_step, w.side_jobs, w.live_image,
		       w.adam_steps32, w.adam_in_reduce, w.adam_prologue, w.adam_prologue_refused, w.mlp_r32, w.mlp_r32a, w.mlp_regs, w.mlp_fast, w.mlp_prio, w.listgrad_in_mlp, w.mlp_layerwise,
		       w.mlp_regw, w.mlp_variant_forced, w.mlp_variant[0], w.mlp_variant[1], w.mlp_variant[2], w.wgrad_rows, w.mlp_fwd_lds, w.fuse_oneblob);
	}
	return 0;
}
