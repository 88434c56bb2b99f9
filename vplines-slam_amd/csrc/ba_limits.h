// Limits that the device layout (ba_types.h) and the plain C++ headers the host-only checks include share.
#pragma once

namespace vpl {

constexpr int NF = 11;                 // WINDOW_SIZE + 1 frames
constexpr int NC = 171;                // cam dims
constexpr int NV = 72;                 // vis dims
constexpr int MAXKEEP = 80;           // new prior dim after MARGIN_OLD: <= 10*6 + 9 + 6 = 75

}  // namespace vpl
