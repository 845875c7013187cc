// lora_keys.hpp -- kohya-ss / LyCORIS LoRA files: module name <-> dump-tree entry, and the header-level plan of a file.  Host only, no HIP.
//
// A kohya file names a module after its *diffusers* path: "lora_unet_" / "lora_te_" + the path with '_' for '.'.  The map is derived by rule and built the way
// dump_name_of_checkpoint_key is: for every conv / Linear entry of the model, its CompVis key (checkpoint_key) is renamed to the diffusers module path
// (the fixed SD v1 renaming below), '.' becomes '_', the prefix is put in front, and module names are looked up in the resulting table.  Nothing parses
// underscores backwards.  The CompVis-style spelling some tools write -- the CompVis key itself with '_' for '.' -- is a second name of the same entry.
// Pinned line by line against tests/golden/kohya_lora_keys.txt.
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "safetensors_reader.hpp"

namespace sdmi {

// The kohya module name of the conv / Linear weight `dump_name` ("unet/.../weight", "clip/.../weight"); false for anything else: a bias, a norm, an
// embedding table, the VAE, a ControlNet, an unknown name.  *compvis (may be null): the CompVis-style spelling (for the text encoder: the same name).
bool lora_module_name(const std::string& dump_name, std::string* kohya, std::string* compvis = nullptr);

// What the plan needs to know of one weight entry of the model
struct LoraEntryDesc {
    std::string name;      // dump name
    int kind;              // 0 conv [cout, cin, kh, kw], 1 Linear [in, out]; anything else is never a target
    int64_t dims[4];
    bool padded;           // a conv_in stored with padded input channels: no target
};

class LoraKeyTable {
public:
    explicit LoraKeyTable(const std::vector<LoraEntryDesc>& entries);   // both spellings of every entry that has a module name
    int find(const std::string& module) const;                           // index into `entries`, -1: no entry of this model
    size_t size() const { return n_entries_; }

private:
    std::map<std::string, int> index_;
    size_t n_entries_ = 0;
};

enum { kLoraUnet = 1, kLoraTe = 2, kLoraSkipUnknown = 1 };   // SDMI_LORA_UNET / _TE, SDMI_LORA_SKIP_UNKNOWN

// One target of a file: the entry, the factorisation, and the factors where the mapping holds them.
// kind 0 (LoRA / LoCon): f[0] = lora_down.weight, f[1] = lora_up.weight.  kind 1 (LoHa): f[0] = hada_w1_b, f[1] = hada_w1_a, f[2] = hada_w2_b, f[3] = hada_w2_a
// (each pair in the order down, up: w_b [r, in] is read as a down factor, w_a [out, r] as an up factor).
struct LoraFileTarget {
    int entry;
    int kind;
    int dtype;             // of all its factors: 0 F32, 1 F16, 2 BF16
    int rank;
    double alpha;          // the file's scalar widened exactly; rank when the file has none
    const StTensor* f[4];
    std::string module;
};

struct LoraFilePlan {
    std::vector<LoraFileTarget> targets;   // in the order the modules first appear in the header
    std::vector<std::string> skipped;      // module names no entry of the model answers to (kLoraSkipUnknown)
};

// Everything that can be checked without a device, before anything is uploaded.  Throws sdmi::Error:
//   SDMI_ERR_UNSUPPORTED  a key kind that is not built (lora_mid / hada_t1 / hada_t2, lokr_*, dora_scale, diff / diff_b, anything unrecognised), a dtype other than
//                         F32 / F16 / BF16, a rank above 256, a padded conv_in, a module no entry of the model answers to (unless kLoraSkipUnknown) -- the first
//                         offending key is named;
//   SDMI_ERR_WEIGHTS      a module with half its factors, a shape that does not fit the entry, a non-finite alpha, two modules naming one entry -- the key is named;
//   SDMI_ERR_INVALID      `which` selects nothing.
// Modules of the half `which` leaves out are passed over.
LoraFilePlan lora_plan_file(const std::vector<StTensor>& tensors, const std::vector<LoraEntryDesc>& entries, int which, int flags);

}  // namespace sdmi
