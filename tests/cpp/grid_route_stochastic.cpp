// grid_route_stochastic.cpp -- the grid encoding's two routes with stochastic_interpolation set, over the argument ranges of
// grid_route_table.cpp (switch sets, grids, batch sizes, callers and options), each compared with the route of the same grid without the key.
// Host code only: constructing a GridEncoding touches no GPU.
//
// Linear and Smoothstep grids: the forward kernel is that of the plain grid; hit lists are never recorded, the list-fed gradient kernel is
// never chosen and the fused MLP kernel's list-order tail never granted (list elements carry all 2^D corners with their weights); the
// gradient family is the plain grid's except Lists -> BitPlanes; the route says `stochastic` exactly where it names a gradient kernel.
// Nearest returns before the flag is read (grid.h:279-282): its routes equal the plain grid's field by field.
// Prints one line of counts and "ok"; a mismatch prints the case and exits with 1.
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>
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
struct Extra { uint32_t dims, levels, F, log2_t, base; uint32_t alignment; bool fp32; };
static const Extra EXTRAS[] = {
	{3, 16, 4, 22, 16, 0, false}, {2, 6, 8, 24, 16, 0, false}, {3, 6, 2, 18, 8, 16, false}, {3, 8, 2, 18, 8, 16, false}, {3, 6, 2, 18, 8, 0, false},
	{3, 8, 2, 18, 8, 0, true}, {2, 8, 4, 15, 16, 0, true},
};
static const uint32_t BATCHES[] = {4000, 4096, 1u << 14, (1u << 16) - 64, 1u << 16, 1u << 18};
static const GradientMode MODES[] = {GradientMode::Ignore, GradientMode::Overwrite, GradientMode::Accumulate};
static const GridMaxLevel MAX_LEVELS[] = {GridMaxLevel::None, GridMaxLevel::Scalar, GridMaxLevel::PerSample};
static const char* INTERPOLATIONS[] = {"Linear", "Smoothstep", "Nearest"};

struct Case { bool fused, input_gradients; GradientMode mode; GridMaxLevel max_level; bool x_contiguous, lists_current; };
struct Routes { GridForwardRoute f; GridBackwardRoute b; };

static Routes routes(GridEncoding& enc, const Switches& sw, uint32_t n, const Case& c) {
	static float per_sample_stub; // (only ever compared with nullptr)
	enc.set_max_level(c.max_level == GridMaxLevel::Scalar ? 0.5f : 1000.f);
	enc.set_max_level_gpu(c.max_level == GridMaxLevel::PerSample ? &per_sample_stub : nullptr);
	const GridFacts g = enc.facts();
	Routes r;
	r.f = grid_forward_route(g, sw, n, c.fused, c.input_gradients, c.fused ? c.mode != GradientMode::Ignore : true);
	r.b = grid_backward_route(g, sw, r.f, c.lists_current, n, c.fused ? GridDyForm::Records : GridDyForm::Rows, c.input_gradients, c.mode, enc.max_level_state(), c.x_contiguous);
	return r;
}

static bool same_forward(const GridForwardRoute& a, const GridForwardRoute& b) {
	return a.planned == b.planned && a.kernel == b.kernel && a.recorded == b.recorded && a.lds == b.lds && a.plane_features == b.plane_features;
}
static bool same_backward(const GridBackwardRoute& a, const GridBackwardRoute& b) {
	return a.dy == b.dy && a.plane_features == b.plane_features && a.record_planes == b.record_planes && a.kernel == b.kernel && a.binned == b.binned && a.tune == b.tune &&
	       a.prologue == b.prologue && a.stochastic == b.stochastic && a.tail == b.tail && a.list_tail.level_mask == b.list_tail.level_mask && a.list_tail.n_levels == b.list_tail.n_levels &&
	       a.tail_bytes == b.tail_bytes;
}

static Json grid_config(const char* type, const char* hash, const char* interpolation, uint32_t levels, uint32_t F, uint32_t log2_t, uint32_t base, bool stochastic) {
	Json j = Json::object();
	j["otype"] = "Grid";
	j["type"] = type;
	j["hash"] = hash;
	j["interpolation"] = interpolation;
	j["n_levels"] = levels;
	j["n_features_per_level"] = F;
	j["log2_hashmap_size"] = log2_t;
	j["base_resolution"] = base;
	j["per_level_scale"] = 1.5f;
	if (stochastic) j["stochastic_interpolation"] = true;
	return j;
}

int main() {
	for (const auto& sw : SWITCH_SETS) if (sw[0]) unsetenv(sw[0]);
	std::vector<Case> cases;
	for (int fused = 1; fused >= 0; --fused) for (int ig = 0; ig < 2; ++ig) for (GradientMode mode : MODES) for (GridMaxLevel ml : MAX_LEVELS) for (int xc = 1; xc >= 0; --xc) for (int cur = 1; cur >= 0; --cur) {
		cases.push_back(Case{fused != 0, ig != 0, mode, ml, xc != 0, cur != 0});
	}
	size_t total = 0, nearest = 0, lists_replaced = 0, records_declined = 0, tails_declined = 0, lists_recorded_plain = 0, stochastic_routes = 0;
	int failures = 0;
	for (const auto& set : SWITCH_SETS) {
		if (set[0]) setenv(set[0], set[1], 1);
		switches_reload();
		const Switches sw = switches();
		const auto grid = [&](uint32_t dims, const char* type, const char* hash, const char* interpolation, uint32_t levels, uint32_t F, uint32_t log2_t, uint32_t base, uint32_t alignment, bool fp32) {
			std::unique_ptr<Encoding> ep = create_encoding(dims, grid_config(type, hash, interpolation, levels, F, log2_t, base, false), alignment, fp32);
			std::unique_ptr<Encoding> es = create_encoding(dims, grid_config(type, hash, interpolation, levels, F, log2_t, base, true), alignment, fp32);
			GridEncoding& plain = dynamic_cast<GridEncoding&>(*ep);
			GridEncoding& stoch = dynamic_cast<GridEncoding&>(*es);
			const bool is_nearest = std::string{interpolation} == "Nearest";
			if (!stoch.facts().stochastic || plain.facts().stochastic) { printf("facts() does not carry the key\n"); ++failures; }
			std::vector<uint32_t> batches(std::begin(BATCHES), std::end(BATCHES));
			batches.push_back(grid_hit_max_samples(plain.meta()));
			batches.push_back(grid_hit_max_samples(plain.meta()) + 64);
			for (uint32_t n : batches) for (const Case& c : cases) {
				if (c.fused && n % BATCH_SIZE_GRANULARITY != 0) continue; // (Model::check_batch throws)
				const Routes p = routes(plain, sw, n, c), s = routes(stoch, sw, n, c);
				++total;
				bool ok;
				if (is_nearest) {
					++nearest;
					ok = same_forward(p.f, s.f) && same_backward(p.b, s.b) && !s.b.stochastic;
				} else {
					const GridGradientKernel want = p.b.kernel == GridGradientKernel::Lists ? GridGradientKernel::BitPlanes : p.b.kernel;
					ok = s.f.kernel == p.f.kernel && s.f.planned && s.f.lds == p.f.lds && s.f.plane_features == p.f.plane_features;
					ok = ok && s.f.recorded != GridRecorded::HitLists &&
					     (p.f.recorded == GridRecorded::Nothing) == (s.f.recorded == GridRecorded::Nothing); // bit planes wherever the plain grid records anything
					ok = ok && s.b.kernel != GridGradientKernel::Lists && s.b.kernel == want && !s.b.tail && s.b.tail_bytes == 0 && s.b.list_tail.gvals == nullptr;
					ok = ok && s.b.stochastic == (s.b.kernel != GridGradientKernel::None) && s.b.dy != GridDyForm::Records;
					ok = ok && (s.b.kernel != GridGradientKernel::BitPlanes || s.b.binned == plain.facts().any_binned);
					// the forms dL/dy may take: the plain grid's, or planes where that takes records
					ok = ok && s.b.dy == (p.b.dy == GridDyForm::Records ? GridDyForm::Planes : p.b.dy);
					lists_recorded_plain += p.f.recorded == GridRecorded::HitLists;
					lists_replaced += p.b.kernel == GridGradientKernel::Lists;
					records_declined += p.b.dy == GridDyForm::Records;
					tails_declined += p.b.tail;
					stochastic_routes += s.b.stochastic;
				}
				if (!ok && ++failures <= 20) {
					printf("%s=%s %uD %s/%s/%s F=%u T=2^%u L=%u fp32=%d n=%u fused=%d ig=%d mode=%d max_level=%d xc=%d cur=%d: plain fwd %d/%d bwd %d dy %d tail %d -- stochastic fwd %d/%d bwd %d dy %d tail %d flag %d\n",
					       set[0] ? set[0] : "default", set[0] ? set[1] : "", dims, type, hash, interpolation, F, log2_t, levels, (int)fp32, n, (int)c.fused, (int)c.input_gradients, (int)c.mode,
					       (int)c.max_level, (int)c.x_contiguous, (int)c.lists_current, (int)p.f.kernel, (int)p.f.recorded, (int)p.b.kernel, (int)p.b.dy, (int)p.b.tail, (int)s.f.kernel,
					       (int)s.f.recorded, (int)s.b.kernel, (int)s.b.dy, (int)s.b.tail, (int)s.b.stochastic);
				}
			}
		};
		for (const char* interpolation : INTERPOLATIONS) {
			for (uint32_t dims : DIMS) for (uint32_t F : FEATURES) for (const Kind& k : KINDS) for (uint32_t log2_t : LOG2_T) grid(dims, k.type, k.hash, interpolation, 8, F, log2_t, 16, 0, false);
			for (const Extra& x : EXTRAS) grid(x.dims, "Hash", "CoherentPrime", interpolation, x.levels, x.F, x.log2_t, x.base, x.alignment, x.fp32);
		}
		if (set[0]) unsetenv(set[0]);
	}
	// the binned grid of tests/test_grid_stochastic_gpu.py is the smallest with a binned level: 2-D, dense, one level of eight features --
	// 129^2 entries are 9 chunks of 2048 (binned from 9 on without scatter records), 128^2 are 8
	for (uint32_t base : {129u, 128u}) {
		Json j = grid_config("Dense", "CoherentPrime", "Linear", 1, 8, 19, base, true);
		std::unique_ptr<Encoding> e = create_encoding(2, j, 0, false);
		const GridFacts g = dynamic_cast<GridEncoding&>(*e).facts();
		if (g.any_binned != (base == 129u) || !g.scatter_levels_ok) { printf("base resolution %u: any_binned %d, levels_ok %d\n", base, (int)g.any_binned, (int)g.scatter_levels_ok); ++failures; }
	}
	printf("%zu cases, %zu of them Nearest; plain grids: %zu record hit lists, %zu take the list-fed kernel, %zu take records, %zu are granted the tail; %zu stochastic routes\n", total, nearest,
	       lists_recorded_plain, lists_replaced, records_declined, tails_declined, stochastic_routes);
	if (failures) { printf("%d mismatches\n", failures); return 1; }
	// the walk is not trivial: each thing the stochastic route declines does occur for the plain grids
	if (!lists_recorded_plain || !lists_replaced || !records_declined || !tails_declined || !stochastic_routes || !nearest) { printf("a declined route never occurred\n"); return 1; }
	printf("ok\n");
	return 0;
}
