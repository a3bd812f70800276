// mlp_train_plan_table.cpp -- which fused training kernel mlp_train_plan chooses, and over how many workgroups, for every combination of
// switch set, network, batch size, input / dL/dx form, loss and option listed below.  Host code only: the library loads without a device.
//
// Per case the program asks what model.h asks, in model.h's order -- is there a fused kernel for n (mlp_train_any_kernel), can the OneBlob
// encoding be evaluated in the kernel (mlp_train_oneblob_in_kernel), are the context matrices compact (mlp_train_compact_context, with the
// Trainer's conditions), then the plan -- and the answer is "-" (no fused step), "noob" (OneBlob not in the kernel: the model encodes into
// rows, another case) or "<family>[/c]:<workgroups = slabs>" (/c: compact context matrices; none:0: no kernel takes the request).
// The cases are nested loops, and so is the output: each level's list of answers is written with runs ("X x5": five in a row), given a
// name where it first occurs and referred to by that name from then on --
//   R<i> = the answers for the batch sizes BATCHES;          F<i> = R's over the forms FORMS (those the input width allows);
//   T<i> = F's over gradients {yes, no} x LOSSES;             D<i> = T's over OUTPUTS x ACTIVATIONS x OUTPUT_ACTIVATIONS;
//   S <switch set> = D's over IN_WIDTHS x WIDTHS x HIDDEN.
// The expected output is tests/golden/mlp_train_plan_table.txt.
#include "../../include/tcnn_amd.h"
#include "../../tiny-cuda-nn_amd/csrc/model.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

using namespace tcnn_amd;

struct Form { const char* name; uint32_t x_plane_f, oneblob_bins; bool dL_dx; uint32_t dx_plane_f, dx_record_dims; };
// what fused_encode / fused_mlp_and_scatter can hand to the MLP kernel: the encoded batch as rows or as level planes of F features, dL/dx
// not wanted, as rows, as level planes or as scatter records (4 k + 2 F <= 16); OneBlob in the kernel (never with dL/dx)
static const Form FORMS[] = {
	{"rows/-", 0, 0, false, 0, 0}, {"rows/rows", 0, 0, true, 0, 0},
	{"planes2/rows", 2, 0, true, 0, 0}, {"planes4/rows", 4, 0, true, 0, 0}, {"planes8/rows", 8, 0, true, 0, 0},
	{"planes2/planes2", 2, 0, true, 2, 0}, {"planes4/planes4", 4, 0, true, 4, 0}, {"planes8/planes8", 8, 0, true, 8, 0},
	{"rows/planes2", 0, 0, true, 2, 0}, {"rows/planes4", 0, 0, true, 4, 0}, {"rows/planes8", 0, 0, true, 8, 0},
	{"planes2/records2x2", 2, 0, true, 2, 2}, {"planes4/records4x2", 4, 0, true, 4, 2}, {"planes2/records2x3", 2, 0, true, 2, 3},
	{"rows/records2x2", 0, 0, true, 2, 2}, {"rows/records4x2", 0, 0, true, 4, 2}, {"rows/records2x3", 0, 0, true, 2, 3},
	{"oneblob32/-", 0, 32, false, 0, 0}, {"oneblob64/-", 0, 64, false, 0, 0}, {"oneblob128/-", 0, 128, false, 0, 0},
};
// L2 / RelativeL2 with and without data_pdf; dL/dy from the caller with the output written (training_step) and without (backward())
struct LossCase { const char* name; LossType loss; bool external, data_pdf, out; };
static const LossCase LOSSES[] = {
	{"L2", LossType::L2, false, false, true}, {"L2+pdf", LossType::L2, false, true, true}, {"RelL2", LossType::RelativeL2, false, false, true},
	{"RelL2+pdf", LossType::RelativeL2, false, true, true}, {"ext", LossType::L2, true, false, true}, {"ext-noout", LossType::L2, true, false, false},
};
static const char* SWITCH_SETS[][2] = { // the default, each A/B switch, and every instantiated (NB, NW, MAXT) of k_mlp_train forced
	{nullptr, nullptr}, {"TCNN_AMD_MLP_REGS", "0"}, {"TCNN_AMD_MLP_R32", "0"}, {"TCNN_AMD_MLP_R32A", "0"}, {"TCNN_AMD_MLP_R32A", "1"}, {"TCNN_AMD_MLP_FAST", "0"},
	{"TCNN_AMD_MLP_REGW", "0"},
	{"TCNN_AMD_MLP_VARIANT", "1,8,8"}, {"TCNN_AMD_MLP_VARIANT", "2,4,8"}, {"TCNN_AMD_MLP_VARIANT", "2,4,16"}, {"TCNN_AMD_MLP_VARIANT", "1,4,16"}, {"TCNN_AMD_MLP_VARIANT", "1,4,32"},
	{"TCNN_AMD_MLP_VARIANT", "1,8,16"}, {"TCNN_AMD_MLP_VARIANT", "1,8,32"},
};
static const uint32_t IN_WIDTHS[] = {16, 32, 64, 128}, WIDTHS[] = {64, 128}, HIDDEN[] = {1, 2, 3, 4, 8};
// 1 - 32 outputs: the counts on both sides of the values the kernels compare with (4 live outputs, 16 and 32 padded ones)
static const uint32_t OUTPUTS[] = {1, 3, 4, 5, 16, 17, 32};
static const char* ACTIVATIONS[] = {"ReLU", "None", "Tanh"};
static const char* OUTPUT_ACTIVATIONS[] = {"None", "Sigmoid"};
static const uint32_t BATCHES[] = {256 * 9, 1u << 14, 1u << 17, (1u << 17) + 256, 1u << 18, 1u << 21, 1u << 22, (1u << 22) + 256};

static const char* family(MlpTrainKernel k) {
	switch (k) {
	case MlpTrainKernel::R32ob: return "r32ob";
	case MlpTrainKernel::R32w: return "r32w";
	case MlpTrainKernel::R32: return "r32";
	case MlpTrainKernel::R32a: return "r32a";
	case MlpTrainKernel::Regs: return "regs";
	case MlpTrainKernel::Train: return "train";
	default: return "none";
	}
}

// what the model asks once per step, before it knows the request
struct Queries { bool any_kernel, compact_context, oneblob_in_kernel[3]; }; // oneblob_in_kernel: for 32, 64, 128 bins
static Queries queries(const MlpDesc& d, uint32_t n) {
	Queries q{};
	q.any_kernel = mlp_train_any_kernel(d, n);
	q.compact_context = mlp_train_compact_context(d, n) && d.out_width == 16; // NetworkWithInputEncoding::fused_compact_context_supported
	for (int i = 0; i < 3; ++i) q.oneblob_in_kernel[i] = mlp_train_oneblob_in_kernel(d, n, 32u << i);
	return q;
}

static std::string answer(const MlpDesc& d, uint32_t n, const Queries& q, const Form& f, const LossCase& l, bool gradients, uint32_t dims) {
	if (!q.any_kernel) return "-";
	if (f.oneblob_bins && !q.oneblob_in_kernel[f.oneblob_bins / 64]) return "noob";
	MlpTrainRequest r;
	r.n = n;
	r.x_plane_features = f.x_plane_f;
	r.oneblob_bins = f.oneblob_bins;
	r.oneblob_dims = f.oneblob_bins ? d.in_width / f.oneblob_bins : 0u;
	r.dims = dims;
	r.loss = l.loss;
	r.external_dL_dy = l.external;
	r.data_pdf = l.data_pdf;
	r.out = l.out;
	r.dL_dx = f.dL_dx;
	r.dx_plane_features = f.dx_plane_f;
	r.dx_record_dims = f.dx_record_dims;
	r.gradients = gradients;
	r.compact_context = !l.external && gradients && q.compact_context; // Trainer::training_step
	const MlpTrainPlan p = mlp_train_plan(d, r);
	return std::string{family(p.ok ? p.kernel : MlpTrainKernel::None)} + (r.compact_context ? "/c:" : ":") + std::to_string(p.ok ? p.grid : 0u);
}

// a level's list, with runs, under the name it got where it first occurred (printed there)
static std::string named(char level, const std::vector<std::string>& items) {
	static std::map<std::string, std::string> names[128];
	static size_t count[128];
	std::string text;
	for (size_t i = 0, j; i < items.size(); i = j) {
		for (j = i + 1; j < items.size() && items[j] == items[i]; ++j) {}
		text += (i ? " " : "") + items[i] + (j - i > 1 ? " x" + std::to_string(j - i) : "");
	}
	std::string& name = names[(int)level][text];
	if (name.empty()) {
		name = level + std::to_string(++count[(int)level]);
		printf("%s = %s\n", name.c_str(), text.c_str());
	}
	return name;
}

int main() {
	for (const auto& sw : SWITCH_SETS) if (sw[0]) unsetenv(sw[0]);
	constexpr size_t N_BATCHES = sizeof(BATCHES) / sizeof(BATCHES[0]);
	size_t cases = 0;
	for (const auto& sw : SWITCH_SETS) {
		if (sw[0]) setenv(sw[0], sw[1], 1);
		switches_reload(); // the process switches, from this environment (as create_from_config does)
		std::vector<std::string> per_shape;
		for (uint32_t in_w : IN_WIDTHS) for (uint32_t w : WIDTHS) for (uint32_t h : HIDDEN) {
			std::vector<std::string> per_net;
			for (uint32_t dims : OUTPUTS) for (const char* act : ACTIVATIONS) for (const char* oact : OUTPUT_ACTIVATIONS) {
				Json net = Json::object();
				net["otype"] = "FullyFusedMLP";
				net["n_input_dims"] = in_w;
				net["n_output_dims"] = dims;
				net["n_neurons"] = w;
				net["n_hidden_layers"] = h;
				net["activation"] = act;
				net["output_activation"] = oact;
				const Network network{net}; // (its constructor touches no GPU)
				const MlpDesc& d = network.desc();
				Queries q[N_BATCHES];
				for (size_t i = 0; i < N_BATCHES; ++i) q[i] = queries(d, BATCHES[i]);
				std::vector<std::string> per_option;
				for (int gradients = 1; gradients >= 0; --gradients) for (const LossCase& l : LOSSES) {
					std::vector<std::string> per_form;
					for (const Form& f : FORMS) {
						if (f.oneblob_bins && in_w % f.oneblob_bins != 0) continue; // OneBlob: bins x dims inputs
						std::vector<std::string> per_batch;
						for (size_t i = 0; i < N_BATCHES; ++i) per_batch.push_back(answer(d, BATCHES[i], q[i], f, l, gradients != 0, dims));
						cases += N_BATCHES;
						per_form.push_back(named('R', per_batch));
					}
					per_option.push_back(named('F', per_form));
				}
				per_net.push_back(named('T', per_option));
			}
			per_shape.push_back(named('D', per_net));
		}
		std::string text;
		for (size_t i = 0, j; i < per_shape.size(); i = j) {
			for (j = i + 1; j < per_shape.size() && per_shape[j] == per_shape[i]; ++j) {}
			text += " " + per_shape[i] + (j - i > 1 ? " x" + std::to_string(j - i) : "");
		}
		printf("S %s =%s\n", sw[0] ? (std::string{sw[0] + 9} + "=" + sw[1]).c_str() : "default", text.c_str());
		if (sw[0]) unsetenv(sw[0]);
	}
	printf("%zu cases\n", cases);
	return 0;
}
