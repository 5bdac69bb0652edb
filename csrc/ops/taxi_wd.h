// hopsx: geometry of the Chicago-taxi wide & deep model that the training kernel (taxi_step.hip) and the
// evaluation kernel (taxi_eval.hip) must agree on.  Each kernel keeps its own LDS map, tile sizes and Args.
#pragma once

namespace taxi_wd {

constexpr int NWIDE = 13;
constexpr int D0 = 3, D1 = 100, D2 = 70, D3 = 48, D4 = 34;  // dense input + hidden widths (logits: 1)

// the 13 wide columns (models/widedeep.py wide_cardinalities): 4 buckets, 2 vocabularies, hour, day, month,
// 2 census tracts, 2 community areas
constexpr int CARD[NWIDE] = {10, 10, 10, 10, 1010, 1010, 24, 31, 12, 2000, 2000, 80, 80};

constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }

// fp32 LDS region both kernels lay out identically (float offsets): the hidden layers' biases, each padded
// to whole 16-wide output tiles, then the logits weight row w4 (zero beyond D4), F_W4_END its end
constexpr int F_B0 = 0, F_B1 = F_B0 + 16 * cdiv(D1, 16), F_B2 = F_B1 + 16 * cdiv(D2, 16),
              F_B3 = F_B2 + 16 * cdiv(D3, 16), F_W4 = F_B3 + 16 * cdiv(D4, 16), F_W4_END = F_W4 + 16 * cdiv(D4, 16);

}  // namespace taxi_wd
