// grid_nd_levels.cpp -- what a grid encoding of 1, 5, 6 or 7 input dimensions is made of, printed for tests/test_grid_nd_host.py to compare
// with the numpy restatement (tests/grid_nd_reference.py).  Host code only: constructing a GridEncoding touches no GPU.
//
//   grid_nd_levels <dims> <fp32: 0|1> '<encoding json>'
// prints
//   n_params <n> padded <width> any_binned <0|1> levels_ok <0|1>
//   level <l> offset <o> size <s> scale <float bits, hex> hashed <0|1> stride <s0> .. <s6> chunks <c> binned <0|1>     (one per level)
//   route <n> <forward kernel>/<recorded>/<gradient kernel>[+binned]   for a module's forward + backward of n = 256, 512 and 1024 rows,
//   under the default switches and under TCNN_AMD_GRID_SCATTER=atomic ("route-atomic")
// or "error <message>" where the constructor refuses the grid.
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace tcnn_amd;

static std::string route(GridEncoding& enc, const Switches& sw, uint32_t n) {
	const GridFacts g = enc.facts();
	const GridForwardRoute f = grid_forward_route(g, sw, n, false, false, true);
	const GridBackwardRoute b = grid_backward_route(g, sw, f, true, n, GridDyForm::Rows, false, GradientMode::Overwrite, enc.max_level_state(), true);
	static const char* kernels[] = {"rows", "planes", "p2r"}, *recorded[] = {"-", "bits", "lists"}, *gradient[] = {"-", "atomic", "scratch32", "bitplanes", "lists"};
	return std::string{kernels[(int)f.kernel]} + "/" + recorded[(int)f.recorded] + "/" + gradient[(int)b.kernel] + (b.binned ? "+binned" : "");
}

int main(int argc, char** argv) {
	if (argc != 4) return 2;
	const uint32_t dims = (uint32_t)atoi(argv[1]);
	const bool fp32 = atoi(argv[2]) != 0;
	unsetenv("TCNN_AMD_GRID_SCATTER");
	try {
		std::unique_ptr<Encoding> e = create_encoding(dims, Json::parse(argv[3]), 0, fp32);
		GridEncoding& enc = dynamic_cast<GridEncoding&>(*e);
		const GridMeta& m = enc.meta();
		const GridFacts g = enc.facts();
		printf("n_params %zu padded %u any_binned %d levels_ok %d\n", enc.n_params(), enc.padded_output_width(), g.any_binned ? 1 : 0, g.scatter_levels_ok ? 1 : 0);
		for (uint32_t l = 0; l < m.n_levels; ++l) {
			const GridLevel& lv = m.levels[l];
			uint32_t bits;
			memcpy(&bits, &lv.scale, 4);
			printf("level %u offset %u size %u scale %08x hashed %u stride", l, lv.offset, lv.size, bits, lv.hashed);
			for (uint32_t d = 0; d < GRID_MAX_DIMS; ++d) printf(" %u", lv.stride[d]);
			printf(" chunks %u binned %u\n", lv.scatter_n_chunks, lv.scatter_binned);
		}
		for (int atomic = 0; atomic < 2; ++atomic) {
			if (atomic) setenv("TCNN_AMD_GRID_SCATTER", "atomic", 1);
			switches_reload();
			const Switches sw = switches();
			for (uint32_t n : {256u, 512u, 1024u}) printf("%s %u %s\n", atomic ? "route-atomic" : "route", n, route(enc, sw, n).c_str());
		}
	} catch (const std::exception& ex) {
		printf("error %s\n", ex.what());
	}
	return 0;
}
