// leaf_text.cpp -- the leaf function that leafjit.cpp generates for a voice, for tests/test_prim_chains.py (TEST INFRASTRUCTURE).
//
// The host-logic simulator has no run-time compiler, so it never generates a voice's source.  This program runs the same host
// code on the CPU: it reads graphs in the C ABI's terms from standard input, lowers each, asks BankMatcher for the voice at
// every output row and prints one JSON line per row: whether a generated voice kernel would take it (jit), its leaves (log2_p),
// its varying parameters per leaf (k) and the text of generate_leaf_source -- what FR_JIT_DUMP shows on the device inside
// jit_bank_<hash>.hip.
//
//   graph <sparkle: 0|1> <n_slots> <fma fold: 0|1>     n <handle> <primitive kind>     e <from> <to> <from_slot> <to_slot>     end
//
// Build: g++ -std=c++17 -O1 -ffp-contract=off -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o leaf_text leaf_text.cpp -ldl
#include <cstdio>
#include <iostream>
#include <string>

#include "../../libfriendship_amd/csrc/graph.cpp"
#include "../../libfriendship_amd/csrc/match.cpp"
#include "../../libfriendship_amd/csrc/leafjit.cpp"

using namespace fr;

static std::string json_string(const std::string &s) {
    std::string out = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') { out += '\\'; out += c; }
        else if (c == '\n') out += "\\n";
        else if (c == '\t') out += "\\t";
        else out += c;
    }
    return out + "\"";
}

int main() {
    std::string word;
    while (std::cin >> word) {
        if (word != "graph") { std::fprintf(stderr, "expected 'graph', got '%s'\n", word.c_str()); return 2; }
        int sparkle = 0, fma = 1;
        uint32_t n_slots = 0;
        std::cin >> sparkle >> n_slots >> fma;
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
        BankMatcher bm(fg, 20, true, true);
        for (uint32_t row = 0; row < n_slots; ++row) {
            VoiceMatch vm;
            if (!bm.try_voice(fg.outputs[row], vm) || !vm.jit) { std::printf("{\"jit\":false}\n"); continue; }
            LeafSource ls = generate_leaf_source(vm.shape, vm.varying, vm.literal_bits, vm.alias, fg.sparkle, fma != 0);
            std::printf("{\"jit\":true,\"k\":%u,\"log2_p\":%u,\"text\":%s}\n", ls.k, vm.log2_p, json_string(ls.text).c_str());
        }
    }
    return 0;
}
