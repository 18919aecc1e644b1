// Stand-alone check of pack_root_rows (lut_ldpc_amd/csrc/hip/lut_program.hpp), built and run by tests/test_root_rows_cpu.py:
//   root_rows_check random          random root / top tables, every pair of input alphabets out of 2, 4, 8, 16
//   root_rows_check trees <file>    the variable trees of a designed code (the reference's text form), every class of degree >= 3
// Every (ch, top) nibble of the packed rows must equal the byte table's entry, labels the table does not hold must read 0, every
// entry of the scaled top table must be 4 x the original, and tables outside the form must be refused.
#include "lut_program.hpp"

#include <cstdio>
#include <fstream>
#include <random>
#include <sstream>

using namespace lutldpc;

static int fails = 0;
#define EXPECT(c, ...) do { if (!(c)) { fails++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static int ilog2(int k) { int s = 0; while ((1 << s) < k) s++; return s; }

// rows / top4 against the byte tables they were packed from
static long check_pair(const std::vector<uint8_t> &root, int shr, const std::vector<uint8_t> &top, const char *what) {
    std::vector<uint8_t> rows, top4;
    const bool ok = pack_root_rows(root.data(), root.size(), shr, top.data(), top.size(), rows, top4);
    EXPECT(ok, "%s: refused", what);
    if (!ok) return 0;
    EXPECT(rows.size() == (size_t)kRootRowsBytes && top4.size() == top.size(), "%s: sizes %zu %zu", what, rows.size(), top4.size());
    long checked = 0;
    for (int ch = 0; ch < 16; ch++) {
        uint64_t row = 0;
        for (int b = 0; b < 8; b++) row |= (uint64_t)rows[(size_t)(ch * 8 + b)] << (8 * b);      // the word as the device reads it (little-endian)
        for (int t = 0; t < 16; t++) {
            const size_t i = (size_t)t | ((size_t)ch << shr);
            const int want = (t < (1 << shr) && i < root.size()) ? root[i] : 0;                  // absent labels read 0
            const int got = (int)((row >> (4 * t)) & 15u);
            EXPECT(got == want, "%s: row %d nibble %d = %d, table says %d", what, ch, t, got, want);
            checked++;
        }
    }
    for (size_t i = 0; i < top.size(); i++) EXPECT(top4[i] == 4 * top[i], "%s: top4[%zu] = %d, top = %d", what, i, top4[i], top[i]);
    return checked;
}

static void run_random() {
    std::mt19937 rng(12345);
    long checked = 0;
    for (int kt : {2, 4, 8, 16})            // alphabet of the tree's top inner node (first input of the root)
        for (int kc : {2, 4, 8, 16})        // channel alphabet (second input)
            for (int ko : {2, 4, 8, 16})    // alphabet the root writes
                for (int rep = 0; rep < 4; rep++) {
                    std::vector<uint8_t> root((size_t)(kt * kc)), top((size_t)(kt * kt));
                    for (auto &x : root) x = (uint8_t)(rng() % (unsigned)ko);
                    for (auto &x : top) x = (uint8_t)(rng() % (unsigned)kt);
                    if (rep == 0) { root.back() = (uint8_t)(ko - 1); root.front() = (uint8_t)(ko - 1); top.back() = (uint8_t)(kt - 1); }    // the corners: bits 60-63 of the last row, nibble 0 of row 0
                    char what[64];
                    std::snprintf(what, sizeof(what), "random top %d cha %d out %d #%d", kt, kc, ko, rep);
                    checked += check_pair(root, ilog2(kt), top, what);
                }
    // tables outside the form are refused
    std::vector<uint8_t> rows, top4, root(256, 3), top(256, 1);
    root[77] = 16;
    EXPECT(!pack_root_rows(root.data(), root.size(), 4, top.data(), top.size(), rows, top4), "a root label of 16 was packed");
    root[77] = 3;
    EXPECT(!pack_root_rows(root.data(), root.size(), 5, top.data(), top.size(), rows, top4), "a 32-label input was packed");
    EXPECT(!pack_root_rows(root.data(), root.size(), 3, top.data(), top.size(), rows, top4), "32 channel labels were packed");
    top[5] = 16;
    EXPECT(!pack_root_rows(root.data(), root.size(), 4, top.data(), top.size(), rows, top4), "a top label without a column was packed");
    std::printf("random: %ld nibbles checked\n", checked);
}

static void run_trees(const char *path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string txt = ss.str();
    TreeArray trees;
    std::string err;
    if (!parse_tree_array(txt.c_str(), trees, err)) { EXPECT(false, "parse: %s", err.c_str()); return; }
    long checked = 0, classes = 0;
    for (size_t s = 0; s < trees.size(); s++)
        for (size_t c = 0; c < trees[s].size(); c++) {
            const Tree &t = trees[s][c];
            if (t.type != TT_VAR || t.num_leaves < 3) continue;
            Program P;
            if (!compile_program(t, TT_VAR, t.num_leaves, P, err)) { EXPECT(false, "compile: %s", err.c_str()); continue; }
            // the root and the inner node that feeds it (balanced trees: ROOT(top inner node, channel))
            const TreeNode *root = t.root.get();
            if (!root || root->child.size() != 2 || root->child[0]->is_leaf() || root->child[1]->type != NT_CHA) continue;
            const TreeNode *top = root->child[0].get();
            std::vector<uint8_t> rt, tp;
            for (auto &nt : P.node_tabs) {
                auto &dst = nt.first == root ? rt : tp;
                if (nt.first == root || nt.first == top) dst.assign(P.tables.begin() + nt.second[0], P.tables.begin() + nt.second[0] + nt.second[1]);
            }
            EXPECT(!rt.empty() && !tp.empty(), "set %zu class %zu: tables not found", s, c);
            char what[64];
            std::snprintf(what, sizeof(what), "set %zu degree %d", s, t.num_leaves);
            checked += check_pair(rt, ilog2(root->child[0]->K), tp, what);
            classes++;
        }
    EXPECT(classes > 0, "no variable tree of degree >= 3");
    std::printf("trees: %ld classes, %ld nibbles checked\n", classes, checked);
}

int main(int argc, char **argv) {
    if (argc >= 2 && std::string(argv[1]) == "random") run_random();
    else if (argc >= 3 && std::string(argv[1]) == "trees") run_trees(argv[2]);
    else { std::printf("usage: root_rows_check random | trees <file>\n"); return 2; }
    std::printf(fails ? "%d failures\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
