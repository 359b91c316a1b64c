// rx_egress_limits.h -- the numbers every departure order of the Rx egress shares (rx_depart_order.h, rx_paced_order.h) and their
// kernels are built around.  Constants alone, so that the order headers stay host-only C++11 that a CPU test can include.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdrhip {
constexpr uint64_t RX_EGRESS_DGRAM_BYTES = 512;
constexpr uint32_t RX_EGRESS_WG_DGRAMS = 32;    // datagrams a KR / KP workgroup moves (256 lanes x 4 chunks of 16 bytes)
constexpr size_t RX_EGRESS_MAX_STREAMS = 65535; // (a tag is a uint16_t)
} // namespace sdrhip
