// Per-renderer options through the C++ host mirror (PluginRenderer, friendship_render_ext.h), run by
// tests/test_options_sim.py against a library named by FRIENDSHIP_RENDERER_LIB.  Prints one line per case.
#include <cstdio>
#include <cstdlib>

#include "../../libfriendship_amd/host/friendship.hpp"

using namespace friendship;

static void attempt(const char *lib, const char *label, const render::PluginRenderer::Options &options) {
    try {
        render::PluginRenderer r(lib, FR_MODE_AUTO, -1, FR_SEMANTICS_REFERENCE, 0, FR_CONFIG_SYNC_COMPILE, options);
        Array2 buff = Array2::zeros(1, 4);
        Jagged2 inputs;
        r.fill_buffer(buff, 0, inputs);
        std::printf("%s: ok %s\n", label, r.options_json().c_str());
    } catch (const render::Panic &p) {
        std::printf("%s: status %d %s\n", label, (int)p.status, p.what());
    }
}

int main() {
    const char *lib = std::getenv("FRIENDSHIP_RENDERER_LIB");
    if (!lib) return 2;
    attempt(lib, "plain", {});
    attempt(lib, "short_off", {{"FR_BANK_SHORT", "0"}, {"FR_STAGE_JIT", "force"}});
    attempt(lib, "unknown", {{"FR_NO_SUCH_SWITCH", "1"}});
    attempt(lib, "process_wide", {{"FR_JIT_DUMP", "/tmp"}});
    attempt(lib, "twice", {{"FR_BANK_SHORT", "0"}, {"FR_BANK_SHORT", "1"}});
    return 0;
}
