// K5t: the level passes of a decision tree (Spark 2.4 ml DecisionTreeRegressor / Classifier,
// continuous features) -- binning, the (node, feature, bin) histogram, the split search, the row
// routing and the prediction walk (see tree.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dq4ml {

enum TreeKind : int { TREE_REG = 0, TREE_CLS = 1 };
enum TreeImpurity : int { TREE_VARIANCE = 0, TREE_GINI = 1, TREE_ENTROPY = 2 };

constexpr int kTreeMaxD = 64, kTreeMaxBins = 256, kTreeMaxClasses = 16;
constexpr int kTreeRegWords = 9;             // count, 4 limbs of sum y (exponent e), 4 limbs of sum y^2 (exponent 2e)
constexpr int kTreeLdsBytes = 64 * 1024;     // a block's histogram (see tree.hip for the choice)
constexpr int kTreeThreads = 256;

// One node record of tree_split, f64 [kTreeRecord]:
//  0 feature (-1: no valid split)   1 split bin        2 gain          3 impurity     4 count
//  5 prediction (mean | first maximal class)           6 left count    7 right count
//  8 left impurity   9 right impurity   10 leaf   11 left child is a leaf   12 right child is a leaf
// 13 left prediction   14 right prediction   16.. class counts   32.. left class counts   48.. right
constexpr int kTreeRecord = 64;

// accumulator words of one (node, feature, bin) cell
constexpr int tree_words(int kind, int classes) { return kind == TREE_CLS ? classes : kTreeRegWords; }
// open nodes whose cells fit one block's LDS (0: not even one; the fused pass does not serve the shape)
constexpr int tree_group(int kind, int d, int nb, int classes) {
  return kTreeLdsBytes / (d * nb * tree_words(kind, classes) * (kind == TREE_CLS ? 4 : 8));
}

struct TreeHistArgs {
  const uint8_t* B;  // [n, dpad] bins, row-major
  const int* node;   // [n] open-node slot of the row, -1: dead or in a leaf
  const void* y;     // [n] labels, f32 / f64
  int ydt;
  int64_t n;
  int d, dpad, nb, classes;
  int e;       // TREE_REG: frexp exponent of the largest |y|
  int g0, G;   // the node group of this launch: slots [g0, g0 + G)
};

struct TreeSplitArgs {
  const long long* H;  // [open, d, nb, words]; with feats: [open, m, nb, words]
  const int* nsplit;   // [d] splits of each feature (bins = splits + 1 <= nb)
  int open, d, nb, classes, kind, impurity, e;
  // A forest's per-node feature subsets (forest.hip): feats[open, m] holds, ascending, the feature
  // whose cells sit at each position of the node.  nullptr: all d features, position = feature.
  const int* feats;
  int m;
  long long min_rows;
  double min_gain;
  int force_leaf;   // the level sits at maxDepth
  int child_leaf;   // its children do
};

int tree_blocks(int64_t n);
// B[r, f] = number of thr[f, 0 .. nsplit[f]) below X[f, r] (f64 compare; dead rows and pad bytes 0);
// flag |= 1 when a live row holds a NaN.  X: feature-major f32 / f64, ld >= n; thr: [d, S] f64.
void tree_bin(const void* X, int64_t ld, int d, int64_t n, int xdt, const uint8_t* sel, const double* thr,
              const int* nsplit, int S, int dpad, uint8_t* B, int* flag, int blocks, hipStream_t st);
// H[g0 .. g0 + G) += the cells of the rows whose slot lies in the group (H zeroed by the caller)
void tree_hist(const TreeHistArgs& a, int kind, long long* H, int blocks, hipStream_t st);
// rec[s] = the record of open node s
void tree_split(const TreeSplitArgs& a, double* rec, hipStream_t st);
// node[r] <- tab[node[r]] = (feature | -1, split bin, left slot, right slot); a leaf child's slot is -1
void tree_route(const uint8_t* B, int dpad, int64_t n, const int* tab, int open, int* node, int blocks, hipStream_t st);
// leaf[r] = index of the leaf that row r reaches (x <= thr goes left; -1 for dead rows) in a tree
// of m nodes stored as feat (-1: leaf) / thr / left / right
void tree_predict(const void* X, int64_t ld, int d, int64_t n, int xdt, const uint8_t* sel, const int* feat,
                  const double* thr, const int* left, const int* right, int m, int* leaf, int blocks, hipStream_t st);

}  // namespace dq4ml
