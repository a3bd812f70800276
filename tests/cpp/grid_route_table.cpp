// grid_route_table.cpp -- the grid encoding's forward and backward route (grid_forward_route, grid_backward_route) for every combination of
// switch set, grid, batch size, caller and option listed below.  Host code only: constructing a GridEncoding touches no GPU.
//
// Per case the program plans the forward route, then the backward route of a context with that forward route, and prints
//   <forward kernel>/<recorded>/<dL/dy form>/<gradient kernel>[+binned][/tail][/prologue]
// forward kernel: rows | planes | p2r (planes + transposition); recorded: - | bits | lists; dL/dy: rows | planes<F> | records<per sample>;
// gradient kernel: - (GradientMode::Ignore) | atomic | scratch32 | bitplanes | lists; tail: the fused MLP kernel's tail may write list order
// (all conditions but the item map); prologue: the finalize pass may go to the optimizer's launch where the fused step offers that.
// "none": the case throws -- a fused step whose batch is no multiple of BATCH_SIZE_GRANULARITY (Model::check_batch).
// The cases are nested loops, and so is the output: each level's list of answers is written with runs ("X x5": five in a row), given a
// name where it first occurs and referred to by that name from then on --
//   O<i> = the answers over CALLERS x input gradients {no, yes} x MODES x MAX_LEVELS x x {contiguous, strided} x lists {current, stale};
//   N<i> = O's over the batch sizes (BATCHES, then the grid's grid_hit_max_samples and that + 64);
//   S <switch set> = N's over the grids: DIMS x FEATURES x KINDS x LOG2_T x {half, 8 levels}, then the EXTRA grids.
// The expected output is tests/golden/grid_route_table.txt.
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

using namespace tcnn_amd;

static const char* SWITCH_SETS[][2] = {
	{nullptr, nullptr}, {"TCNN_AMD_GRID_PLANES", "0"}, {"TCNN_AMD_GRID_ROWS_PLANES", "0"}, {"TCNN_AMD_GRID_SCATTER", "atomic"}, {"TCNN_AMD_SCATTER_RECORDS", "0"},
	{"TCNN_AMD_SCATTER_LISTS", "0"}, {"TCNN_AMD_SCATTER_LISTS", "1"}, {"TCNN_AMD_LISTGRAD_IN_MLP", "0"},
};
static const uint32_t DIMS[] = {2, 3, 4}, FEATURES[] = {1, 2, 4, 8}, LOG2_T[] = {12, 15, 19};
struct Kind { const char* type; const char* hash; };
static const Kind KINDS[] = {{"Hash", "CoherentPrime"}, {"Dense", "CoherentPrime"}, {"Tiled", "CoherentPrime"}, {"Hash", "Rng"}};
// (dims, levels, F, log2 T, base resolution, alignment of the consumer, fp32)
struct Extra { uint32_t dims, levels, F, log2_t, base; uint32_t alignment; bool fp32; };
static const Extra EXTRAS[] = {
	{3, 16, 4, 22, 16, 0, false},  // levels of more than 64 chunks: binned
	{2, 6, 8, 24, 16, 0, false},   // more chunks than either LDS path takes
	{3, 6, 2, 18, 8, 16, false},   // 12 features in front of a 16-aligned network: two whole planes of padding
	{3, 8, 2, 18, 8, 16, false},   // ... beside 16 features, no padding
	{3, 6, 2, 18, 8, 0, false},    // (an Encoding module pads to a multiple of F only)
	{3, 8, 2, 18, 8, 0, true}, {2, 8, 4, 15, 16, 0, true}, // fp32
};
static const uint32_t BATCHES[] = {4000, 4096, 1u << 14, (1u << 16) - 64, 1u << 16, 1u << 18};
static const GradientMode MODES[] = {GradientMode::Ignore, GradientMode::Overwrite};
static const GridMaxLevel MAX_LEVELS[] = {GridMaxLevel::None, GridMaxLevel::Scalar, GridMaxLevel::PerSample};

struct Case { bool fused, input_gradients; GradientMode mode; GridMaxLevel max_level; bool x_contiguous, lists_current; };

static std::string answer(GridEncoding& enc, const Switches& sw, uint32_t n, const Case& c) {
	if (c.fused && n % BATCH_SIZE_GRANULARITY != 0) return "none";
	static float per_sample_stub; // (only ever compared with nullptr)
	enc.set_max_level(c.max_level == GridMaxLevel::Scalar ? 0.5f : 1000.f);
	enc.set_max_level_gpu(c.max_level == GridMaxLevel::PerSample ? &per_sample_stub : nullptr);
	const GridFacts g = enc.facts();
	// the fused step prepares parameter gradients unless it ignores them; forward() of a model always does
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

// a level's list, with runs, under the name it got where it first occurred (printed there)
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
		switches_reload(); // the process switches, from this environment (as create_from_config does)
		const Switches sw = switches();
		std::vector<std::string> per_grid;
		const auto grid = [&](uint32_t dims, const Json& config, uint32_t alignment, bool fp32) {
			std::unique_ptr<Encoding> e = create_encoding(dims, config, alignment, fp32);
			GridEncoding& enc = dynamic_cast<GridEncoding&>(*e);
			std::vector<uint32_t> batches(std::begin(BATCHES), std::end(BATCHES));
			batches.push_back(grid_hit_max_samples(enc.meta()));
			batches.push_back(grid_hit_max_samples(enc.meta()) + 64);
			std::vector<std::string> per_batch;
			for (uint32_t n : batches) {
				std::vector<std::string> per_case;
				for (const Case& c : cases) per_case.push_back(answer(enc, sw, n, c));
				total += cases.size();
				per_batch.push_back(named('O', per_case));
			}
			per_grid.push_back(named('N', per_batch));
		};
		for (uint32_t dims : DIMS) for (uint32_t F : FEATURES) for (const Kind& k : KINDS) for (uint32_t log2_t : LOG2_T) grid(dims, grid_config(k.type, k.hash, 8, F, log2_t, 16), 0, false);
		for (const Extra& x : EXTRAS) grid(x.dims, grid_config("Hash", "CoherentPrime", x.levels, x.F, x.log2_t, x.base), x.alignment, x.fp32);
		printf("S %s = %s\n", set[0] ? (std::string{set[0] + 9} + "=" + set[1]).c_str() : "default", runs(per_grid).c_str());
		if (set[0]) unsetenv(set[0]);
	}
	printf("%zu cases\n", total);
	return 0;
}
