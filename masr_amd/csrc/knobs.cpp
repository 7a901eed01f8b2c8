#include "knobs.h"

namespace masr {

Knobs& knobs() {
    static Knobs k;
    return k;
}

#define KNOB(key, field, experimental) {key, #field, &Knobs::field, experimental}
static const KnobInfo TABLE[] = {
    KNOB(1, ffn_variant, false),
    KNOB(5, no_chain, false),
    KNOB(6, rowgemm_small, false),
    KNOB(7, attention_fewq, false),
    KNOB(8, no_ffn_tail, false),
    KNOB(9, no_ffn_head, false),
    KNOB(12, rowgemm_small_blocks, false),
    KNOB(13, ffn_split_blocks, false),
    KNOB(14, attention_fold, false),
    KNOB(15, embed_split, false),
    KNOB(17, gemm_waves, false),
    KNOB(18, conv1_nt, false),
    KNOB(19, hot_weights, false),
    KNOB(20, bf16x3, true),
    KNOB(21, gemm_bf16x3_waves, true),
    KNOB(22, ffn_x3_rotation, true),
    KNOB(23, ffn_packed, false),
    KNOB(24, ffn_dual, true),
    KNOB(25, rowgemm_packed, false),
    KNOB(26, attention_grouped_fold, false),
    KNOB(27, ctc_fused_blocks, false),
    KNOB(28, attention_fewq_wgs, false),
    KNOB(29, few_rows_path, false),
    KNOB(30, split_head, true),
    KNOB(31, efficient_fused, false),
    KNOB(32, beam_lm_cache, false),
    KNOB(33, conv2_mid_fill, false),
    KNOB(34, attn_chain, true),
    KNOB(35, ffn_coop, true),
    KNOB(36, sqz_fused_blocks, false),
    KNOB(37, beam_narrow, false),
    KNOB(39, ffn16, false),
    KNOB(40, conv2_rows, false),
    KNOB(41, conv1_fused, false),
    KNOB(42, embed_rows, false),
    KNOB(43, rnn_mfma_units, false),
};
#undef KNOB
static const int N_KNOBS = sizeof(TABLE) / sizeof(TABLE[0]);

const KnobInfo* knob_info(int index) { return index >= 0 && index < N_KNOBS ? &TABLE[index] : nullptr; }

const KnobInfo* knob_find(int key) {
    for (const KnobInfo& k : TABLE)
        if (k.key == key) return &k;
    return nullptr;
}

int knob_default(const KnobInfo& k) { return Knobs{}.*k.field; }

bool knob_set(int key, int value, Knobs& into) {
    const KnobInfo* k = knob_find(key);
    if (k) into.*k->field = value;
    return k != nullptr;
}

void knobs_reset() { knobs() = Knobs{}; }

}  // namespace masr
