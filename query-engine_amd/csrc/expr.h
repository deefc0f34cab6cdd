// Expression programs: the host compiles a postfix `PhysicalExpr`
// (qeh_expr, include/qeh.h) into a typed register program that every kernel
// interprets with wave-uniform dispatch.  Typing / coercion follows the
// reference exactly (operators.rs:382-709); errors carry the reference's text.
#pragma once

#include <stdint.h>

#include <vector>

#include "../../include/qeh.h"
#include "device_common.h"

namespace qeh {

constexpr int kNS = 8;        // value slots (= max stack depth)
constexpr int kMaxInstr = 40;

enum DevOp : uint8_t {
    D_LOAD = 0,   // dst <- column[a]            (t = column dtype)
    D_LIT,        // dst <- imm / NULL           (t = dtype, flag = is_null)
    D_TOF64,      // dst <- (double) int slot a  (t = source dtype)
    D_ADD, D_SUB, D_MUL, D_DIV, D_MOD,         // t = operand dtype
    D_EQ, D_NE, D_LT, D_LE, D_GT, D_GE,        // t = operand dtype (after coercion)
    D_AND, D_OR, D_NOT, D_NEG
};

struct DevInstr {
    uint8_t op, t, dst, a;
    uint8_t b, flag, pad0, pad1;
    int64_t imm;
};

struct DevProgram {
    int32_t n;            // instructions
    int32_t result_type;  // dtype of slot 0 after the program
    DevInstr ins[kMaxInstr];
};

// Fast path: a single-level AND-list or OR-list of `column CMP literal`
// comparisons (the shape of every predicate in the BASELINE configs).
constexpr int kMaxTerms = 6;
struct PredTerm {
    int32_t col;      // column index
    int32_t ctype;    // compare type: QEH_DT_INT64 or QEH_DT_FLOAT64 (or BOOL)
    int32_t op;       // D_EQ..D_GE with the column on the left
    int32_t _pad;
    int64_t lit;      // int64 literal, or totalOrder key of the double literal
};
struct PredTerms {
    int32_t n;        // 0 = always TRUE (no predicate)
    int32_t is_or;    // 0 = AND-list, 1 = OR-list (non-Kleene, arrow and/or)
    PredTerm t[kMaxTerms];
};

// error bits reported by kernels (atomicOr into a scratch word)
constexpr uint32_t kErrOverflow = 1u;
constexpr uint32_t kErrDiv0 = 2u;
constexpr uint32_t kErrModOverflow = 4u;
constexpr uint32_t kErrSpin = 8u;
constexpr uint32_t kErrExprMask = kErrOverflow | kErrDiv0 | kErrModOverflow;

// Which expression error a launch reports: the reference's first.  evaluate_expr is post-order and
// every operator finishes its whole array (rows in order, NULL rows skipped) before the next one
// starts, so the first error is the minimum of (instruction, row) over the valid rows that raise --
// compile_expr emits in postfix order, and the D_TOF64 it inserts cannot raise.  A lane keeps that
// minimum as a key (pc < kMaxInstr, row < 2^32 by check_column, kind = one kErr* bit) and merges its
// complement with one 64-bit atomicMax into a zeroed word, so that 0 still means "no error".
constexpr uint64_t kNoFirstErr = ~0ull;
__host__ __device__ inline uint64_t first_err_key(int pc, int64_t row, uint32_t kind) {
    return ((uint64_t)pc << 35) | ((uint64_t)row << 3) | kind;
}
// the kErr* bit of the first error in a launch's first-error word (0: none)
inline uint32_t first_err_kind(uint64_t word) { return word ? (uint32_t)(~word & 7u) : 0u; }

// Host side --------------------------------------------------------------------
// Compile `e` over columns of `dtypes`.  Returns QEH_OK or an error status with
// qeh_last_error set to the reference's message.
int compile_expr(const qeh_expr *e, const int32_t *dtypes, int n_cols, DevProgram *out);
// The result type of `e` by the reference's typing alone, no device program: Utf8 columns and
// literals and scalar functions (QEH_EX_SCALAR_FUNCTION) included, which compile_expr refuses.
int type_expr(const qeh_expr *e, const int32_t *dtypes, int n_cols, int32_t *out_type);
// One scalar function's arity check, then its argument-type check (operators.rs:74-259), with the
// reference's messages; *out_type = its result type.
int scalar_fn_type(int func, const int *arg_types, int n_args, int *out_type);
const char *scalar_fn_name(int func);
// True when `e` holds a node the expression program cannot carry and qeh_eval / qeh_filter
// materialise first: a scalar function, or a full-text match (QEH_OP_TSMATCH).
bool expr_has_function(const qeh_expr *e);
// marks[i] != 0: node i is a TO_TSVECTOR / TO_TSQUERY function that is the direct operand of a
// QEH_OP_TSMATCH node -- the only place the two are accepted (they become that side's mode).
// False on a malformed postfix (the typing pass reports it).
bool ts_match_operands(const qeh_expr *e, std::vector<char> *marks);
// The checks of such an operand: arity, then the argument's type (operators.rs:261-297).
int ts_fn_type(int func, const int *arg_types, int n_args, int *out_type);
// Try to lower to the fast term list (only for BOOL-typed predicates).
bool lower_to_terms(const qeh_expr *e, const int32_t *dtypes, int n_cols, PredTerms *out);
// Index of the column a bare Column expression refers to, else -1.
int expr_as_column(const qeh_expr *e);
// Index of the input column whose buffers qeh_eval returns un-owned (owned = 0) for `e`: a bare
// Column, or COALESCE chains whose first arguments end in one (COALESCE is its first argument,
// unchanged).  -1: the result of `e` is a column of its own.
int expr_aliased_column(const qeh_expr *e);
// Columns referenced by an expression (bitmask over <= 64 columns).
uint64_t expr_columns(const qeh_expr *e);

}  // namespace qeh
