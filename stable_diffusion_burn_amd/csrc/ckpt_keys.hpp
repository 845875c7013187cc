// ckpt_keys.hpp -- dump-tree name -> key of an SD v1.x checkpoint in the CompVis layout ("model.diffusion_model.…",
// "first_stage_model.…", "cond_stage_model.transformer.text_model.…", "alphas_cumprod").  Host only, no HIP.
//
// The map is the composition of two things the reference defines: the attribute paths of python/dump.py's StableDiffusion
// (= the checkpoint's keys: the reference loads it with load_state_dict) and the directory names its exporters write
// (python/{stablediffusion,unet,autoencoder,clip}.py).  It is derived by rule -- block index arithmetic and the fixed renames --
// and pinned line by line against tests/golden/sd14_ckpt_keys.txt, which tests/golden/gen_ckpt_keys.py writes by running both.
#pragma once
#include <string>

namespace sdmi {

// false: `dump_name` has no checkpoint source (module metadata such as eps / n_group / n_head, n_steps; an unknown name).
// *transposed: the dump holds [in, out] where the checkpoint holds torch's [out, in] (a Linear weight, python/save.py:19).
bool checkpoint_key(const std::string& dump_name, std::string* key, bool* transposed);

// The inverse: the dump-tree name whose checkpoint_key is `key`; false for any other key (model_ema.*, position_ids ...).  Built from the rules themselves:
// every module path the grammar of checkpoint_key can produce is run through it once (CLIP layers: any index).
bool dump_name_of_checkpoint_key(const std::string& key, std::string* dump_name);

// The LDM "scaled linear" schedule of SD v1.x, what a checkpoint's alphas_cumprod holds: betas = linspace(sqrt(0.00085), sqrt(0.012), n)^2,
// out = float32(cumprod(1 - betas)), every step in f64 in numpy's order of operations (synthetic.py: alphas_cumprod).
void default_alphas_cumprod(float* out, int n);

}  // namespace sdmi
