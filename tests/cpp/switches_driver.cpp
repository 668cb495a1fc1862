// Prints the environment switches of the kernel library (genomeworks_amd/csrc/gwhip_switches.h) as the three readers see
// them in the environment this program is started in: one line per struct. Host only, no GPU.
#include <cstdio>

#include "../../genomeworks_amd/csrc/gwhip_switches.h"

int main()
{
    const gwhip::PoaSwitches p = gwhip::read_poa_switches();
    std::printf("poa debug_flags=%d persistent_grid=%d msa_serial=%d consensus_hbm_only=%d consensus_full_tables=%d\n", p.debug_flags,
                (int)p.persistent_grid, (int)p.msa_serial, (int)p.consensus_hbm_only, (int)p.consensus_full_tables);
    const gwhip::MyersSwitches m = gwhip::read_myers_switches();
    std::printf("myers skip=%d hbm_state=%d group=%d group_lanes=%d mirror_blocks=%d\n", m.skip, (int)m.hbm_state, m.group, m.group_lanes,
                m.mirror_blocks);
    const gwhip::HirschbergSwitches h = gwhip::read_hirschberg_switches();
    std::printf("hirschberg wave=%d levels=%d span=%d span_single_wave=%d\n", h.wave, (int)h.levels, (int)h.span, (int)h.span_single_wave);
    return 0;
}
