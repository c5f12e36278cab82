// voice_proof.cpp -- what the bank matcher proves about a voice, for tests/test_proofs_sim.py (TEST INFRASTRUCTURE).
//
// The host-logic simulator has no run-time compiler, so its plans never hold a shape-matched voice and its fr_plan_json has no
// fast_ok for one.  This program runs the same host code on the CPU: it reads graphs in the C ABI's terms from standard input,
// lowers each, asks BankMatcher for the voice at output row 0 and prints one JSON line per graph: whether a generated voice
// kernel would take it (jit), BankMatcher's fast_ok, and the generated leaf's HAS_MOD1 and FRACT_INPUTS (as input slots).
//
//   graph <sparkle: 0|1> <n_slots>        n <handle> <primitive kind>        e <from> <to> <from_slot> <to_slot>        end
//
// Build: g++ -std=c++17 -O1 -ffp-contract=off -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o voice_proof voice_proof.cpp -ldl
#include <cstdio>
#include <iostream>
#include <string>

#include "../../libfriendship_amd/csrc/graph.cpp"
#include "../../libfriendship_amd/csrc/match.cpp"
#include "../../libfriendship_amd/csrc/leafjit.cpp"

using namespace fr;

int main() {
    std::string word;
    while (std::cin >> word) {
        if (word != "graph") { std::fprintf(stderr, "expected 'graph', got '%s'\n", word.c_str()); return 2; }
        int sparkle = 0;
        uint32_t n_slots = 0;
        std::cin >> sparkle >> n_slots;
        Mirror m;
        m.sparkle = sparkle != 0;
        while (std::cin >> word && word != "end") {
            if (word == "n") {
                uint32_t h; int kind;
                std::cin >> h >> kind;
                fr_effect e{};
                e.kind = kind;
                m.add_node(h, &e);
            } else if (word == "e") {
                fr_edge e{};
                std::cin >> e.from >> e.to >> e.from_slot >> e.to_slot;
                m.add_edge(e);
            } else { std::fprintf(stderr, "unknown record '%s'\n", word.c_str()); return 2; }
        }
        FlatGraph fg = lower(m, n_slots);
        BankMatcher bm(fg, 20, true, false);
        VoiceMatch vm;
        if (!bm.try_voice(fg.outputs[0], vm)) { std::printf("{\"matched\":false}\n"); continue; }
        LeafSource ls;
        if (vm.jit) ls = generate_leaf_source(vm.shape, vm.varying, vm.literal_bits, vm.alias, fg.sparkle, true);
        std::string fract, slots;   // FRACT_INPUTS as input slots; every slot the leaf reads
        for (size_t i = 0; i < vm.shape.input_slots.size(); ++i) {
            slots += (slots.empty() ? "" : ",") + std::to_string(vm.shape.input_slots[i]);
            if ((ls.fract_inputs >> i) & 1u) fract += (fract.empty() ? "" : ",") + std::to_string(vm.shape.input_slots[i]);
        }
        std::printf("{\"matched\":true,\"jit\":%s,\"fast_ok\":%s,\"has_mod1\":%s,\"fract_slots\":[%s],\"input_slots\":[%s],\"k\":%u,\"log2_p\":%u}\n", vm.jit ? "true" : "false",
                    vm.fast_ok ? "true" : "false", ls.has_mod1 ? "true" : "false", fract.c_str(), slots.c_str(), vm.k, vm.log2_p);
    }
    return 0;
}
