// grid_route_table_nd.cpp -- the grid encoding's forward and backward route (grid_forward_route, grid_backward_route) for grids of 1, 5, 6
// and 7 input dimensions: the rows tests/cpp/grid_route_table.cpp would hold for them, in the same notation.  Host code only.
//
// Per case the program plans the forward route, then the backward route of a context with that forward route, and prints
//   <forward kernel>/<recorded>/<dL/dy form>/<gradient kernel>[+binned][/tail][/prologue]
// (see grid_route_table.cpp).  "none": a fused step whose batch is no multiple of BATCH_SIZE_GRANULARITY.  Lists of answers are written
// with runs and named where they first occur:
//   O<i> = the answers over CALLERS x input gradients {no, yes} x MODES x MAX_LEVELS x x {contiguous, strided} x lists {current, stale};
//   N<i> = O's over the batch sizes;
//   S <switch set> = N's over the grids: DIMS x FEATURES x KINDS x LOG2_T x {half, 8 levels, base resolution 4}, then the EXTRA grids.
// The expected output is tests/golden/grid_route_table_nd.txt.
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

using namespace tcnn_amd;

static const char* SWITCH_SETS[][2] = {
	{nullptr, nullptr}, {"TCNN_AMD_GRID_PLANES", "0"}, {"TCNN_AMD_GRID_SCATTER", "atomic"}, {"TCNN_AMD_SCATTER_RECORDS", "0"}, {"TCNN_AMD_SCATTER_LISTS", "1"},
};
static const uint32_t DIMS[] = {1, 5, 6, 7}, FEATURES[] = {1, 2, 4, 8}, LOG2_T[] = {12, 15, 19};
struct Kind { const char* type; const char* hash; };
static const Kind KINDS[] = {{"Hash", "CoherentPrime"}, {"Dense", "CoherentPrime"}, {"Tiled", "CoherentPrime"}, {"Hash", "Rng"}};
// (dims, levels, F, log2 T, base resolution, alignment of the consumer, fp32)
struct Extra { uint32_t dims, levels, F, log2_t, base; uint32_t alignment; bool fp32; };
static const Extra EXTRAS[] = {
	{5, 16, 4, 22, 4, 0, false},   // levels of more than 64 chunks: binned
	{7, 6, 8, 24, 2, 0, false},    // more chunks than either LDS path takes
	{5, 6, 2, 18, 4, 16, false},   // 12 features in front of a 16-aligned network
	{1, 16, 2, 19, 16, 0, false},  // a 1-D signal at the default table size
	{5, 8, 2, 18, 4, 0, true}, {7, 8, 4, 15, 2, 0, true}, // fp32
};
static const uint32_t BATCHES[] = {4000, 4096, 1u << 16, 1u << 18};
static const GradientMode MODES[] = {GradientMode::Ignore, GradientMode::Overwrite};
static const GridMaxLevel MAX_LEVELS[] = {GridMaxLevel::None, GridMaxLevel::Scalar, GridMaxLevel::PerSample};

struct Case { bool fused, input_gradients; GradientMode mode; GridMaxLevel max_level; bool x_contiguous, lists_current; };

static std::string answer(GridEncoding& enc, const Switches& sw, uint32_t n, const Case& c) {
	if (c.fused && n % BATCH_SIZE_GRANULARITY != 0) return "none";
	static float per_sample_stub; // (only ever compared with nullptr)
	enc.set_max_level(c.max_level == GridMaxLevel::Scalar ? 0.5f : 1000.f);
	enc.set_max_level_gpu(c.max_level == GridMaxLevel::PerSample ? &per_sample_stub : nullptr);
	const GridFacts g = enc.facts();
	const GridForwardRoute f = grid_forward_route(g, sw, n, c.fused, c.input_gradients, c.fused ? c.mode != GradientMode::Ignore : true);
	const GridBackwardRoute b = grid_backward_route(g, sw, f, c.lists_current, n, c.fused ? GridDyForm::Records : GridDyForm::Rows, c.input_gradients, c.mode, enc.max_level_state(), c.x_contiguous);
	static const char* kernels[] = {"rows", "planes", "p2r"}, *recorded[] = {"-", "bits", "lists"}, *gradient[] = {"-", "atomic", "scratch32", "bitplanes", "lists"};
	std::string s = std::string{kernels[(int)f.kernel]} + "/" + recorded[(int)f.recorded] + "/";
	if (b.dy == GridDyForm::Rows) s += "rows";
	else if (b.dy == GridDyForm::Planes) s += "planes" + std::to_string(b.plane_features);
	else s += "records" + std::to_string(b.record_planes);
	s += std::string{"/"} + gradient[(int)b.kernel] + (b.binned ? "+binned" : "");
	if (b.tail) s += "/tail";
	const bool lds = b.kernel == GridGradientKernel::BitPlanes || b.kernel == GridGradientKernel::Lists;
	if (c.fused && lds && b.prologue) s += "/prologue";
	return s;
}

static std::string runs(const std::vector<std::string>& items) {
	std::string text;
	for (size_t i = 0, j; i < items.size(); i = j) {
		for (j = i + 1; j < items.size() && items[j] == items[i]; ++j) {}
		text += (i ? " " : "") + items[i] + (j - i > 1 ? " x" + std::to_string(j - i) : "");
	}
	return text;
}
static std::string named(char level, const std::vector<std::string>& items) {
	static std::map<std::string, std::string> names[128];
	static size_t count[128];
	const std::string text = runs(items);
	std::string& name = names[(int)level][text];
	if (name.empty()) {
		name = level + std::to_string(++count[(int)level]);
		printf("%s = %s\n", name.c_str(), text.c_str());
	}
	return name;
}

static Json grid_config(const char* type, const char* hash, uint32_t levels, uint32_t F, uint32_t log2_t, uint32_t base) {
	Json j = Json::object();
	j["otype"] = "Grid";
	j["type"] = type;
	j["hash"] = hash;
	j["n_levels"] = levels;
	j["n_features_per_level"] = F;
	j["log2_hashmap_size"] = log2_t;
	j["base_resolution"] = base;
	j["per_level_scale"] = 1.5f;
	return j;
}

int main() {
	for (const auto& sw : SWITCH_SETS) if (sw[0]) unsetenv(sw[0]);
	std::vector<Case> cases;
	for (int fused = 1; fused >= 0; --fused) for (int ig = 0; ig < 2; ++ig) for (GradientMode mode : MODES) for (GridMaxLevel ml : MAX_LEVELS) for (int xc = 1; xc >= 0; --xc) for (int cur = 1; cur >= 0; --cur) {
		cases.push_back(Case{fused != 0, ig != 0, mode, ml, xc != 0, cur != 0});
	}
	size_t total = 0;
	for (const auto& set : SWITCH_SETS) {
		if (set[0]) setenv(set[0], set[1], 1);
		switches_reload();
		const Switches sw = switches();
		std::vector<std::string> per_grid;
		const auto grid = [&](uint32_t dims, const Json& config, uint32_t alignment, bool fp32) {
			std::unique_ptr<Encoding> e = create_encoding(dims, config, alignment, fp32);
			GridEncoding& enc = dynamic_cast<GridEncoding&>(*e);
			std::vector<std::string> per_batch;
			for (uint32_t n : BATCHES) {
				std::vector<std::string> per_case;
				for (const Case& c : cases) per_case.push_back(answer(enc, sw, n, c));
				total += cases.size();
				per_batch.push_back(named('O', per_case));
			}
			per_grid.push_back(named('N', per_batch));
		};
		for (uint32_t dims : DIMS) for (uint32_t F : FEATURES) for (const Kind& k : KINDS) for (uint32_t log2_t : LOG2_T) grid(dims, grid_config(k.type, k.hash, 8, F, log2_t, 4), 0, false);
		for (const Extra& x : EXTRAS) grid(x.dims, grid_config("Hash", "CoherentPrime", x.levels, x.F, x.log2_t, x.base), x.alignment, x.fp32);
		printf("S %s = %s\n", set[0] ? (std::string{set[0] + 9} + "=" + set[1]).c_str() : "default", runs(per_grid).c_str());
		if (set[0]) unsetenv(set[0]);
	}
	printf("%zu cases\n", total);
	return 0;
}
