// K5r: the level passes of a random forest (Spark 2.4 ml RandomForestRegressor / Classifier,
// continuous features) -- the bagging pass, the histogram of the open nodes of all trees over
// per-node feature subsets, the routing of every tree's node word and the forest's prediction walk
// (see forest.hip).  The split search is tree.hip's, given the subsets (TreeSplitArgs::feats).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tree.h"

namespace dq4ml {

// A row's node word in tree t: -1 (dead, outside the bag, or in a leaf), else
// (bag count << kForestCountShift) | slot, slot = the open node's number in the level, tree-major.
constexpr int kForestCountShift = 24;
constexpr int kForestSlotMask = (1 << kForestCountShift) - 1;
constexpr int kForestMaxCount = 15;  // thresholds of a bag rule; the count fits the word's top bits

// The bag rule, passed by value in the kernarg (as FoldRule is): the count of a row is the number
// of thresholds thr[0 .. k) that its hash reaches.
struct BagRule {
  int k;
  uint32_t thr[kForestMaxCount];
};

// bytes of one slot in a block's LDS: its m x nb cells and its feature mask
constexpr int forest_slot_bytes(int kind, int m, int nb, int classes) {
  return m * nb * tree_words(kind, classes) * (kind == TREE_CLS ? 4 : 8) + 8;
}
// slots whose cells and masks fit one block's LDS (0: not even one)
constexpr int forest_group(int kind, int m, int nb, int classes) {
  return kTreeLdsBytes / forest_slot_bytes(kind, m, nb, classes);
}

struct ForestHistArgs {
  const uint8_t* B;      // [n, dpad] bins, row-major
  const int* node;       // [trees, n] node words, tree-major
  const void* y;         // [n] labels, f32 / f64
  const uint64_t* mask;  // [slots of the level] bit f: feature f is in the slot's subset (<= m bits)
  int ydt;
  int64_t n;
  int d, dpad, nb, classes, m;
  int e;        // TREE_REG: frexp exponent of the largest |y|
  int g0, G;    // the slot group of this launch: slots [g0, g0 + G)
  int t0, t1;   // the trees that own those slots: t0 <= t <= t1
};

// node[t, r] = (c << 24) | t for a live row with c = #{j < k : fold_hash(seeds[t], row_offset + r) >=
// thr[j]} >= 1, else -1
void forest_bag(int64_t n, int64_t row_offset, const uint8_t* sel, const uint64_t* seeds, int trees, const BagRule& rule,
                int* node, int blocks, hipStream_t st);
// H[g0 .. g0 + G) [m][nb][W] += count x the label words of the rows whose word lies in the group, at
// the features of the slot's mask (H zeroed by the caller)
void forest_hist(const ForestHistArgs& a, int kind, long long* H, int blocks, hipStream_t st);
// node[t, r] <- (count bits | tab[slot] child) for every tree; tab as tree_route's, slots of all trees
void forest_route(const uint8_t* B, int dpad, int64_t n, const int* tab, int open, int* node, int trees, int blocks,
                  hipStream_t st);
// out[k, r] = sum over the trees, in tree order, of val[leaf_t(r), k] (k < C <= 16; NaN for dead
// rows); the trees are concatenated in feat (-1: leaf) / thr / left / right (indices into the
// concatenation), root[t] the root of tree t
void forest_predict(const void* X, int64_t ld, int d, int64_t n, int xdt, const uint8_t* sel, const int* feat,
                    const double* thr, const int* left, const int* right, int nodes, const int* root, int trees,
                    const double* val, int C, double* out, int blocks, hipStream_t st);

}  // namespace dq4ml
