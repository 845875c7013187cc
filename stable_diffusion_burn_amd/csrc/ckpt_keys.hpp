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
// The same for a model variant (sdmi_config.variant): 0 = the rule above; 1 = SD 2.x in Stability's layout -- the UNet and the VAE under their v1 keys, the text
// encoder under "cond_stage_model.model." (OpenCLIP: transformer.resblocks.<i>.{ln_1, ln_2, attn.in_proj_weight | in_proj_bias, attn.out_proj, mlp.c_fc, mlp.c_proj},
// token_embedding.weight, positional_embedding, ln_final).  *slice: -1 = the key's whole tensor; 0 / 1 / 2 = its first / second / third block of rows -- the query, key
// and value parts of a fused attn.in_proj_weight [3C, C] / in_proj_bias [3C].
bool checkpoint_key(const std::string& dump_name, int variant, std::string* key, bool* transposed, int* slice);
// The checkpoint family a key set belongs to, decided by the text encoder's final LayerNorm: 1 = SD v1 (CompVis: cond_stage_model.transformer.text_model.final_layer_norm.weight),
// 2 = SD 2.x (cond_stage_model.model.ln_final.weight), 0 = neither key present.
extern const char* const kFamilyKeySd1;
extern const char* const kFamilyKeySd2;

// The inverse: the dump-tree name whose checkpoint_key is `key`; false for any other key (model_ema.*, position_ids ...).  Built from the rules themselves:
// every module path the grammar of checkpoint_key can produce is run through it once (CLIP layers: any index).
bool dump_name_of_checkpoint_key(const std::string& key, std::string* dump_name);

// The LDM "scaled linear" schedule of SD v1.x, what a checkpoint's alphas_cumprod holds: betas = linspace(sqrt(0.00085), sqrt(0.012), n)^2,
// out = float32(cumprod(1 - betas)), every step in f64 in numpy's order of operations (synthetic.py: alphas_cumprod).
void default_alphas_cumprod(float* out, int n);

}  // namespace sdmi
