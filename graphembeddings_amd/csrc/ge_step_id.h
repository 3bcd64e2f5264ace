// ge_step_id.h -- what names a sequence of training steps behind the C ABI: the type-safe corruption tables, the
// triple list the batches are cut from, and the identity the pipeline handle keeps of the records it prepared ahead.
// Pointers and integers only, no HIP: a plain host program can include it (tests/step_identity_check.cpp).
#pragma once
#include <stdint.h>

#include <tuple>

namespace ge {

// The corruption tables of holE.py:267-277 and the counter-based stream that draws from them: type code per table row,
// CSR of type code -> ids, Philox seed, the per-batch subsample size, GE_CORRUPT_*.
struct TypeSampler {
  const int32_t* id_to_type; int64_t N; const int64_t* type_offsets; int32_t n_types; const int32_t* type_ids;
  uint64_t seed; int32_t padded_size, mode;
};

// mode in GE_CORRUPT_*, no negative count: what corrupt_batch_launch and the loops' entry points refuse (ge_capi.hip)
inline bool sampler_ranges_ok(const TypeSampler& ts) {
  return ts.mode >= 0 && ts.mode <= 3 && ts.padded_size >= 0 && ts.n_types >= 0;
}

// Step s of a sequence is the batch of B rows at step_row(first_row, T, B, s) of `triples`, drawn with step key
// global_step0 + s.
struct StepSeq {
  const int32_t* triples; int64_t T, first_row, B; uint64_t global_step0;
};

// Everything a prepared record depends on, and the workspace it lies in.
struct StepIdentity {
  StepSeq seq; TypeSampler ts; int32_t d; int direct, negs; void* workspace;
};

// Two calls read the same source: records prepared for one are good for the other wherever their step numbers meet.
// Every field but the position in the sequence (seq.first_row, seq.global_step0: whether b goes on where a stopped is
// a question of how far a has come, PrepCursor::begin).  Field by field -- the structs have padding.
inline bool same_source(const StepIdentity& a, const StepIdentity& b) {
  const auto key = [](const StepIdentity& i) {
    return std::tie(i.seq.triples, i.seq.T, i.seq.B, i.ts.id_to_type, i.ts.N, i.ts.type_offsets, i.ts.n_types, i.ts.type_ids,
                    i.ts.seed, i.ts.padded_size, i.ts.mode, i.d, i.direct, i.negs, i.workspace);
  };
  return key(a) == key(b);
}

}  // namespace ge
