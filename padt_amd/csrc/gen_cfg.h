// The generation-config slots: the ONE definition of their layout.  ops.gen_cfg_tensor packs these 16 ints (ops.GEN_CFG_FMT) and every
// kernel that takes a `gen_cfg` pointer reads them through this struct; a slot that moves fails the asserts below instead of misreading
// device memory.
// Kept in DEVICE memory so a captured decode graph does not bake them in (HF generation_config.json: repetition_penalty, eos_token_id
// list; padt.py:570-580,717,756).
#pragma once
#include "common.h"
#include <stddef.h>

struct GenCfg {
    float penalty;                     // RepetitionPenaltyLogitsProcessor: score<0 ? score*p : score/p on every id already in the row
    int eos[4];                        // up to 4 EOS ids, -1 = unused
    int do_sample;                     // 0 greedy (arg-max), 1 multinomial sampling (padt.py:740-743) by sample_token_kernel
    unsigned seed;                     // counter-based RNG key (the device step counter, row and table index are the counter)
    float temperature;                 // TemperatureLogitsWarper
    int top_k;                         // TopKLogitsWarper (0 = off)
    float top_p;                       // TopPLogitsWarper (1 = off)
    int write_back;                    // sample_token_kernel overwrites its input rows with the warped scores (l / T, -inf outside the kept set)
    int pad;
    // read by warp_sample_rows_kernel alone (every other kernel stops at `pad`): HF's warpers after top-p, each with its "off" value
    float min_p;                       // MinPLogitsWarper: active when 0 < min_p <= 1 (0 = off)
    float typical_p;                   // TypicalLogitsWarper: active when 0 < typical_p < 1 (1 = off)
    float epsilon_cutoff;              // EpsilonLogitsWarper: active when 0 < epsilon < 1 (0 = off)
    float eta_cutoff;                  // EtaLogitsWarper: active when 0 < epsilon < 1 (0 = off)
};
static_assert(sizeof(GenCfg) == 64, "GenCfg is 16 ints (ops.GEN_CFG_INTS)");
#define PADT_GEN_SLOT(field, slot) static_assert(offsetof(GenCfg, field) == 4 * (slot), "GenCfg." #field " moved: ops.GEN_CFG_FMT packs it in slot " #slot)
PADT_GEN_SLOT(penalty, 0);
PADT_GEN_SLOT(eos, 1);
PADT_GEN_SLOT(do_sample, 5);
PADT_GEN_SLOT(seed, 6);
PADT_GEN_SLOT(temperature, 7);
PADT_GEN_SLOT(top_k, 8);
PADT_GEN_SLOT(top_p, 9);
PADT_GEN_SLOT(write_back, 10);
PADT_GEN_SLOT(pad, 11);
PADT_GEN_SLOT(min_p, 12);
PADT_GEN_SLOT(typical_p, 13);
PADT_GEN_SLOT(epsilon_cutoff, 14);
PADT_GEN_SLOT(eta_cutoff, 15);
#undef PADT_GEN_SLOT

constexpr int GEN_RULES_MAX = 4096;    // ints of the packed rule table of gen_rules_kernel (ops.GEN_RULES_INTS)

// tok is one of the config's listed EOS ids (g is not null)
PADT_DEV bool gen_eos_listed(const GenCfg* g, long tok) {
    bool r = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) r = r || (g->eos[k] >= 0 && tok == (long)g->eos[k]);
    return r;
}
// tok ends a row: the model config's EOS id, or one of the listed ids when there is a generation config
PADT_DEV bool gen_is_eos(const GenCfg* g, long tok, int cfg_eos) {
    bool r = tok == (long)cfg_eos;
    if (g) r = r || gen_eos_listed(g, tok);
    return r;
}
