// gwhip_switches.h -- the environment switches of the kernel library (libgwhip.so), in one place.
//
//   name                      values            effect
//   GWHIP_DEBUG               integer (atoi)    the POA kernels' debug selectors, poa_debug_flags.h; unset or 0: production kernels
//   GWHIP_POA_PERSISTENT      0                 POA: always one block per window, no persistent grid
//   GWHIP_MSA_SERIAL          1                 POA, MSA output: the serial HBM routine, not the wave-wide one with its marks in LDS
//   GWHIP_CONSENSUS_SERIAL    1                 POA, consensus output: the HBM-only kernel
//                             2                 ... the LDS kernel, but never with the small tables
//   GWHIP_MYERS_SKIP          integer (atoi)    Myers: debug_skip of the banded kernels (parts of the work left out, timing only)
//   GWHIP_MYERS_HBM_STATE     1                 Myers: the HBM-state kernel even where the LDS one fits
//   GWHIP_MYERS_GROUP         0 / 1             Myers: the group kernel never / whenever its LDS tables fit
//   GWHIP_MYERS_GROUP_LANES   6, 8, 16, 32, 64  Myers: lanes per pair of the group kernel (any other value is ignored)
//   GWHIP_MIRROR_BLOCKS       integer >= 1      Myers: widest grid of the kernel that mirrors results to the host; default 16.
//                                               Read once per process (the first call), unlike all the others
//   GWHIP_HIRSCHBERG_WAVE     0 / 1             Hirschberg: one wavefront per pair never / whenever its LDS fits
//   GWHIP_HIRSCHBERG_LEVELS   0                 Hirschberg: no level-by-level kernel, depth-first only
//   GWHIP_HIRSCHBERG_SPAN     0                 Hirschberg: no span path for long single pairs
//                             1                 ... the span path with one wavefront per half at every level
//
// Where one character decides, it is the value's first; anything else, the empty string included, is as good as unset.
// Each entry point reads its switches once, at its top, on every call: the tests change them between calls.
// Plain host C++, no HIP (tests/cpp/switches_driver.cpp prints the three structs).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

namespace gwhip
{

struct PoaSwitches
{
    int32_t debug_flags;       // GWHIP_DEBUG
    bool persistent_grid;      // not GWHIP_POA_PERSISTENT=0
    bool msa_serial;           // GWHIP_MSA_SERIAL=1
    bool consensus_hbm_only;   // GWHIP_CONSENSUS_SERIAL=1
    bool consensus_full_tables; // GWHIP_CONSENSUS_SERIAL=2
};

struct MyersSwitches
{
    int32_t skip;         // GWHIP_MYERS_SKIP
    bool hbm_state;       // GWHIP_MYERS_HBM_STATE=1
    int32_t group;        // GWHIP_MYERS_GROUP: 0 never, 1 always, -1 the kernel's own choice
    int32_t group_lanes;  // GWHIP_MYERS_GROUP_LANES: 6, 8, 16, 32 or 64; 0 the kernel's own choice
    int32_t mirror_blocks; // GWHIP_MIRROR_BLOCKS
};

struct HirschbergSwitches
{
    int32_t wave;          // GWHIP_HIRSCHBERG_WAVE: 0 never, 1 whenever it fits, -1 the kernel's own choice
    bool levels;           // not GWHIP_HIRSCHBERG_LEVELS=0
    bool span;             // not GWHIP_HIRSCHBERG_SPAN=0
    bool span_single_wave; // GWHIP_HIRSCHBERG_SPAN=1
};

namespace switches_detail
{
inline char first_char(const char* name)
{
    const char* e = std::getenv(name);
    return e ? e[0] : '\0';
}
inline int32_t integer(const char* name)
{
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : 0;
}
inline int32_t zero_one_or_unset(const char* name)
{
    const char c = first_char(name);
    return c == '0' ? 0 : (c == '1' ? 1 : -1);
}
} // namespace switches_detail

inline PoaSwitches read_poa_switches()
{
    using namespace switches_detail;
    PoaSwitches s;
    s.debug_flags           = integer("GWHIP_DEBUG");
    s.persistent_grid       = first_char("GWHIP_POA_PERSISTENT") != '0';
    s.msa_serial            = first_char("GWHIP_MSA_SERIAL") == '1';
    s.consensus_hbm_only    = first_char("GWHIP_CONSENSUS_SERIAL") == '1';
    s.consensus_full_tables = first_char("GWHIP_CONSENSUS_SERIAL") == '2';
    return s;
}

inline MyersSwitches read_myers_switches()
{
    using namespace switches_detail;
    MyersSwitches s;
    s.skip        = integer("GWHIP_MYERS_SKIP");
    s.hbm_state   = first_char("GWHIP_MYERS_HBM_STATE") == '1';
    s.group       = zero_one_or_unset("GWHIP_MYERS_GROUP");
    const int32_t v = integer("GWHIP_MYERS_GROUP_LANES");
    s.group_lanes = (v == 6 || v == 8 || v == 16 || v == 32 || v == 64) ? v : 0;
    static const int32_t mirror_blocks = std::getenv("GWHIP_MIRROR_BLOCKS") ? std::max(1, integer("GWHIP_MIRROR_BLOCKS")) : 16;
    s.mirror_blocks = mirror_blocks;
    return s;
}

inline HirschbergSwitches read_hirschberg_switches()
{
    using namespace switches_detail;
    HirschbergSwitches s;
    s.wave             = zero_one_or_unset("GWHIP_HIRSCHBERG_WAVE");
    s.levels           = first_char("GWHIP_HIRSCHBERG_LEVELS") != '0';
    s.span             = first_char("GWHIP_HIRSCHBERG_SPAN") != '0';
    s.span_single_wave = first_char("GWHIP_HIRSCHBERG_SPAN") == '1';
    return s;
}

} // namespace gwhip
