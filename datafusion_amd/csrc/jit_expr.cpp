// Query compiler, expressions: one IR node -> C++ text over the skeleton's
// helpers (jit_skeleton.hip), with its literal and string slots. The kernel
// bodies that call this are in jit_kernels.cpp.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "jit_gen.h"
#include "rem_literal.h"

namespace dfmi {
namespace jit {

namespace {

const char* cmp_sym(int op) {
    static const char* s[] = {"==", "!=", "<", "<=", ">", ">="};
    return s[op];
}
const char* math_sym(int op) {
    static const char* s[] = {"+", "-", "*", "/"};
    return s[op - DFMI_OP_PLUS];
}

// Modulus by an integer literal: the reciprocal path (irem_lit) unless
// DFMI_DIAG=1 DFMI_REM_LITERAL=0 forces the general one (A/B runs; read once).
const bool g_rem_literal = [] {
    const char* e = getenv("DFMI_DIAG") ? getenv("DFMI_REM_LITERAL") : nullptr;
    return !e || atoi(e) != 0;
}();

bool is_float(int t) { return t == DFMI_TYPE_FLOAT32 || t == DFMI_TYPE_FLOAT64; }

// Casts num::cast can never reject: int -> float, Float32 -> Float64, and an
// integer into a type holding all of its values.
bool cast_total(int from, int to) {
    // DFMI_FLAG_EXT_CAST_ANY: Boolean <-> numeric always fits, a string may not parse
    if (from == DFMI_TYPE_UTF8) return false;
    if (from == DFMI_TYPE_BOOLEAN || to == DFMI_TYPE_BOOLEAN) return true;
    if (is_float(to)) return !is_float(from) || type_width(from) <= type_width(to);
    if (is_float(from)) return false;
    const int wf = type_width(from), wt = type_width(to);
    if (is_signed_int(from) == is_signed_int(to)) return wt >= wf;
    return !is_signed_int(from) && wt > wf;  // unsigned into a wider signed type
}

// Unsigned type integer math is done in (Rust's wrapping +, -, * on every
// width; C++ signed overflow is undefined and u16 * u16 would promote to int).
const char* math_type(int t) { return type_width(t) == 8 ? "u64" : "u32"; }

// Validity of a node that is null if either operand is: "true" when both are
// statically valid.
std::string both_valid(const Val& a, const Val& b) {
    return a.n != "true" || b.n != "true" ? "(" + a.n + " && " + b.n + ")" : "true";
}

}  // namespace

bool may_introduce_nulls(const dfmi_program* p) {
    for (const IrNode& n : p->ir)
        if (n.kind == IR_CAST && !cast_total(p->ir[n.l].type, n.type)) return true;
    return false;
}

const char* ctype(int t) {
    switch (t) {
        case DFMI_TYPE_INT8: return "i8";
        case DFMI_TYPE_INT16: return "i16";
        case DFMI_TYPE_INT32: return "i32";
        case DFMI_TYPE_INT64: return "i64";
        case DFMI_TYPE_UINT8: return "u8";
        case DFMI_TYPE_UINT16: return "u16";
        case DFMI_TYPE_UINT32: return "u32";
        case DFMI_TYPE_FLOAT32: return "float";
        case DFMI_TYPE_FLOAT64: return "double";
        default: return "u64";
    }
}

// ------------------------------------------------------------- generator
// one slot per literal node (no sharing of equal values: the source text,
// and so the compiled kernel, must not depend on literal values)
int Gen::lit(uint64_t b) {
    LitPool& L = X.lits;
    if (L.n_lits >= 32) throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "query compiler: too many literals"};
    L.bits[L.n_lits] = b;
    return L.n_lits++;
}
int Gen::lit_at(const dfmi_program* p, int node, int which, uint64_t b) {
    const auto key = std::make_tuple(p, node, which);
    const auto it = lit_slots.find(key);
    if (it != lit_slots.end()) return it->second;
    return lit_slots[key] = lit(b);
}
int Gen::strlit(const std::string& s) {
    LitPool& L = X.lits;
    if (L.n_str >= 8 || L.str_bytes + (int)s.size() > 256)
        throw Fail{DFMI_ERR_NOT_IMPLEMENTED, "query compiler: string literals too long"};
    L.str_off[L.n_str] = L.str_bytes;
    L.str_len[L.n_str] = (int)s.size();
    memcpy(L.str + L.str_bytes, s.data(), s.size());
    L.str_bytes += (int)s.size();
    return L.n_str++;
}

// validity of Utf8 slot u's value in `row` (a filtered batch has no nulls)
std::string Gen::utf8_valid(int u) const {
    return filtered_cols ? "true" : "dfmi::utf8_valid(A, " + std::to_string(u) + ", row)";
}

// column value for the current row k (inside a per-k loop)
Val Gen::col(const IrNode& n) {
    const std::string id = std::to_string(X.slot_of_col(n.col));
    Val r;
    if (n.type == DFMI_TYPE_BOOLEAN) {
        r.v = "(((bw" + id + "[k] >> lane) & 1) != 0)";
    } else {
        r.v = "c" + id + "[k]";
    }
    r.n = (!filtered_cols && X.col_nullable(n.col)) ? "(((vw" + id + "[k] >> lane) & 1) != 0)" : "true";
    return r;
}

// Literal slot read as a value of type t (the slot holds the raw bits:
// Float32 in the low 32 bits, integers sign/zero-extended).
static std::string lit_value(int t, int slot) {
    const std::string a = "A.lits[" + std::to_string(slot) + "]";
    if (t == DFMI_TYPE_FLOAT64) return "__builtin_bit_cast(double, " + a + ")";
    if (t == DFMI_TYPE_FLOAT32) return "__builtin_bit_cast(float, (u32)" + a + ")";
    return "((" + std::string(ctype(t)) + ")" + a + ")";
}

// Utf8 ordering compare (DFMI_FLAG_EXT_UTF8_ORDER): bytewise, unsigned, a
// proper prefix first; nulls by cmp_opt as the numeric compares. A literal
// on the left is compared from the column's side with the mirrored
// operator (cmp_opt still sees the operands in their own order).
Val Gen::emit_utf8_order(const dfmi_program* p, const IrNode& n, const IrNode& L, const IrNode& R, int ord_base,
                          const char* act) {
    std::ostream& o = *out;
    const int op = n.op;
    const std::string v = t();
    if (L.kind == IR_LIT && R.kind == IR_LIT) {  // folded: unsigned bytes, then the lengths
        const size_t m = std::min(L.str.size(), R.str.size());
        int c = m ? memcmp(L.str.data(), R.str.data(), m) : 0;
        if (c == 0) c = L.str.size() < R.str.size() ? -1 : (L.str.size() > R.str.size() ? 1 : 0);
        const bool r = op == DFMI_OP_LT ? c < 0 : op == DFMI_OP_LT_EQ ? c <= 0 : op == DFMI_OP_GT ? c > 0 : c >= 0;
        o << "    const bool " << v << " = " << (r ? "true" : "false") << ";\n";
        return Val{v, "true"};
    }
    const Val a = emit(p, n.l, ord_base, act);  // validity only
    const Val b = emit(p, n.r, ord_base, act);
    const std::string H = std::to_string(X.ord_h);
    std::string res;
    if (L.kind == IR_COL && R.kind == IR_COL) {
        res = "dfmi::utf8_cmp_col<" + std::to_string(op) + ", " + H + ">(A, " + std::to_string(X.slot_of_utf8(L.col)) +
              ", " + std::to_string(X.slot_of_utf8(R.col)) + ", row)";
    } else {
        const bool lit_left = L.kind == IR_LIT;
        const IrNode& C = lit_left ? R : L;
        const IrNode& S = lit_left ? L : R;
        static const int mirror[] = {DFMI_OP_GT, DFMI_OP_GT_EQ, DFMI_OP_LT, DFMI_OP_LT_EQ};
        const std::string mop = std::to_string(lit_left ? mirror[op - DFMI_OP_LT] : op);
        const int u = X.slot_of_utf8(C.col);
        const int sl = strlit(S.str);
        if (tile_pre && X.ord_pre) {
            const std::string arr = "uo" + std::to_string(pre_ord.size());
            pre_ord.emplace_back(arr, u, sl);
            res = "dfmi::utf8_ord_tile<" + mop + ">(" + arr + ", k)";
        } else {
            res = "dfmi::utf8_cmp_lit<" + mop + ", " + H + ">(A, " + std::to_string(u) + ", row, " +
                  std::to_string(sl) + ", A0.str + A0.str_off[" + std::to_string(sl) + "])";
        }
    }
    if (a.n == "true" && b.n == "true")
        o << "    const bool " << v << " = " << res << ";\n";
    else
        o << "    const bool " << v << " = dfmi::cmp_opt<" << op << ">(" << a.n << ", " << b.n << ", " << res << ");\n";
    return Val{v, "true"};
}

// The checks of a Divide-style operator on an evaluated, non-null row: a zero
// divisor, and for signed integers MIN / -1 (`overflow`: its ERRK_ name).
void Gen::emit_div_checks(const char* act, const std::string& valid, const Val& a, const Val& b, int ty, int ord,
                          const char* overflow) {
    std::ostream& o = *out;
    const std::string ct = ctype(ty);
    o << "    if ((" << act << ") && " << valid << ") {\n"
      << "      if ((" << b.v << ") == (" << ct << ")0) dfmi::report_err(A.err, " << ord
      << ", row, dfmi::ERRK_DIV_ZERO);\n";
    if (is_signed_int(ty))
        o << "      else if ((" << b.v << ") == (" << ct << ")-1 && (" << a.v << ") == dfmi::int_min<" << ct
          << ">()) dfmi::report_err(A.err, " << ord << ", row, dfmi::" << overflow << ");\n";
    o << "    }\n";
}

// Emit node i of program p; act = C++ bool expression "row is evaluated".
Val Gen::emit(const dfmi_program* p, int i, int ord_base, const char* act) {
    std::ostream& o = *out;
    const IrNode& n = p->ir[i];
    if (n.kind == IR_COL) {
        if (n.type == DFMI_TYPE_UTF8) {  // value only inside Utf8 compares; validity for IS NULL
            if (filtered_cols || !X.col_nullable(n.col)) return Val{"", "true"};
            return Val{"", utf8_valid(X.slot_of_utf8(n.col))};
        }
        if (!type_width(n.type) && n.type != DFMI_TYPE_BOOLEAN)
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED,
                       std::string("device path: ") + type_debug(n.type) + " column in an expression"};
        return col(n);
    }
    if (n.kind == IR_LIT) {
        if (n.type == DFMI_TYPE_UTF8) return Val{"", "true"};
        if (!type_width(n.type))
            throw Fail{DFMI_ERR_NOT_IMPLEMENTED, std::string("device path: ") + type_debug(n.type) + " literal"};
        return Val{lit_value(n.type, lit_at(p, i, 0, n.bits)), "true"};
    }
    if (n.kind == IR_ISNULL) {  // extension: the operand's validity, never null
        const Val a = emit(p, n.l, ord_base, act);
        if (a.n == "true") return Val{n.op == 0 ? "false" : "true", "true"};
        const std::string v = t();
        o << "    const bool " << v << " = " << (n.op == 0 ? "!" : "") << "(" << a.n << ");\n";
        return Val{v, "true"};
    }
    if (n.kind == IR_CAST) {  // extension: arrow cast kernel, unfit values -> null
        const Val a = emit(p, n.l, ord_base, act);
        const int from = p->ir[n.l].type, to = n.type;
        if (from == to) return a;
        const std::string v = t();
        if (from == DFMI_TYPE_UTF8) {
            // DFMI_FLAG_EXT_CAST_ANY: the column's bytes parsed (str::parse); what
            // does not parse is a null. Shaped like the Divide arm: the limit
            // report for evaluated, non-null rows, then the value.
            const std::string ct = to == DFMI_TYPE_BOOLEAN ? "bool" : ctype(to);
            const int u = X.slot_of_utf8(p->ir[n.l].col);
            o << "    " << ct << " " << v << ";\n    bool " << v << "_l = false;\n"
              << "    const bool " << v << "_n = (" << act << ")" << (a.n != "true" ? " && (" + a.n + ")" : "")
              << " && dfmi::utf8_parse<" << ct << ">(A, " << u << ", row, " << v << ", " << v << "_l);\n";
            if (is_float(to))
                o << "    if (" << v << "_l) dfmi::report_err(A.err, " << ord_base + n.ordinal
                  << ", row, dfmi::ERRK_CAST_DIGITS" << (to == DFMI_TYPE_FLOAT32 ? "_F32" : "") << ");\n";
            o << "    if (!" << v << "_n) " << v << " = (" << ct << ")0;\n";
            return Val{v, v + "_n"};
        }
        if (from == DFMI_TYPE_BOOLEAN) {  // true -> 1, false -> 0; a null stays a null (zero slot)
            o << "    const " << ctype(to) << " " << v << " = (" << ctype(to) << ")((" << (a.n != "true" ? "(" + a.n + ") && " : "")
              << "(" << a.v << ")) ? 1 : 0);\n";
            return Val{v, a.n};
        }
        if (to == DFMI_TYPE_BOOLEAN) {  // x != 0: NaN is true, -0.0 false
            o << "    const bool " << v << " = " << (a.n != "true" ? "(" + a.n + ") && " : "") << "((" << a.v
              << ") != (" << ctype(from) << ")0);\n";
            return Val{v, a.n};
        }
        o << "    " << ctype(to) << " " << v << ";\n";
        if (cast_total(from, to)) {
            o << "    (void)dfmi::num_cast<" << ctype(to) << ">(" << a.v << ", " << v << ");\n";
            if (a.n != "true") o << "    if (!(" << a.n << ")) " << v << " = (" << ctype(to) << ")0;\n";
            return Val{v, a.n};
        }
        o << "    const bool " << v << "_n = dfmi::num_cast<" << ctype(to) << ">(" << a.v << ", " << v << ")"
          << (a.n != "true" ? " && (" + a.n + ")" : "") << ";\n";
        o << "    if (!" << v << "_n) " << v << " = (" << ctype(to) << ")0;\n";
        return Val{v, v + "_n"};
    }
    if (n.kind == IR_FN) {  // extension: built-in function -- null if any argument is (zero slot), no errors
        const Val a = emit(p, n.l, ord_base, act);
        const Val b = n.r >= 0 ? emit(p, n.r, ord_base, act) : Val{"", "true"};
        const std::string ct = ctype(n.type);
        const std::string v = t();
        o << "    " << ct << " " << v << " = dfmi::fn_" << scalar_fn_name(n.fn) << "<" << ct << ">(" << a.v
          << (n.r >= 0 ? ", " + b.v : "") << ");\n";
        if (a.n == "true" && b.n == "true") return Val{v, "true"};
        const std::string nn = a.n == "true" ? b.n : (b.n == "true" ? a.n : "(" + a.n + " && " + b.n + ")");
        o << "    const bool " << v << "_n = " << nn << ";\n";
        o << "    if (!" << v << "_n) " << v << " = (" << ct << ")0;\n";
        return Val{v, v + "_n"};
    }
    const int ord = ord_base + n.ordinal;
    if (n.rt_code) {
        // the reference evaluates both children before failing here
        try {
            emit(p, n.l, ord_base, act);
            emit(p, n.r, ord_base, act);
        } catch (const Fail&) {
        }
        if (n.type == DFMI_TYPE_BOOLEAN) return Val{"false", "true"};
        return Val{"((" + std::string(ctype(n.type)) + ")0)", "true"};
    }
    const int op = n.op;
    const IrNode& L = p->ir[n.l];
    if (L.type == DFMI_TYPE_UTF8 && op <= DFMI_OP_GT_EQ) {  // extension: Utf8 =, !=, <, <=, >, >=
        const IrNode& R = p->ir[n.r];
        if (op >= DFMI_OP_LT) return emit_utf8_order(p, n, L, R, ord_base, act);
        const bool eq = op == DFMI_OP_EQ;
        const std::string v = t();
        if (L.kind == IR_LIT && R.kind == IR_LIT) {
            o << "    const bool " << v << " = " << (((L.str == R.str) == eq) ? "true" : "false") << ";\n";
        } else if (L.kind == IR_COL && R.kind == IR_COL) {
            const int u = X.slot_of_utf8(L.col), w = X.slot_of_utf8(R.col);
            o << "    bool " << v << ";\n    { const bool a_ = " << utf8_valid(u) << ", b_ = " << utf8_valid(w) << ";\n"
              << "      const bool e_ = (a_ && b_) ? dfmi::utf8_eq_col(A, " << u << ", " << w << ", row) : (!a_ && !b_);\n"
              << "      " << v << " = " << (eq ? "e_" : "!e_") << "; }\n";
        } else {
            const IrNode& C = L.kind == IR_COL ? L : R;
            const IrNode& S = L.kind == IR_COL ? R : L;
            const int u = X.slot_of_utf8(C.col);
            const int sl = strlit(S.str);
            const std::string vu = utf8_valid(u);
            if (tile_pre) {
                const std::string arr = "uq" + std::to_string(pre_eq.size());
                pre_eq.emplace_back(arr, u, sl);
                o << "    const bool " << v << "_e = " << vu << " && " << arr << "[k];\n";
            } else {
                o << "    const bool " << v << "_e = " << vu << " && dfmi::utf8_eq_lit(A, " << u << ", row, " << sl
                  << ", A0.str + A0.str_off[" << sl << "]);\n";
            }
            o << "    const bool " << v << " = " << (eq ? "" : "!") << v << "_e;\n";
        }
        return Val{v, "true"};
    }
    const Val a = emit(p, n.l, ord_base, act);
    const Val b = emit(p, n.r, ord_base, act);
    const bool nul = a.n != "true" || b.n != "true";
    if (op == DFMI_OP_AND || op == DFMI_OP_OR) {
        const std::string v = t();
        o << "    const bool " << v << "_n = " << both_valid(a, b) << ";\n";
        o << "    const bool " << v << " = " << v << "_n && (" << a.v << (op == DFMI_OP_AND ? " && " : " || ")
          << b.v << ");\n";  // null -> zero value bit (append_null)
        return Val{v, nul ? v + "_n" : "true"};
    }
    // same-typed operands (anything else carries rt_code): compare / compute
    // in the operand type -- iN/uN wrap, Float32 and Float64 round once per
    // operator (-ffp-contract=off)
    const int ty = L.type;
    const bool f = is_float(ty);
    const std::string ct = ctype(ty);
    const std::string v = t();
    if (op <= DFMI_OP_GT_EQ) {
        const std::string cmp = "(" + a.v + ") " + cmp_sym(op) + " (" + b.v + ")";
        if (nul) {
            o << "    const bool " << v << " = dfmi::cmp_opt<" << op << ">(" << a.n << ", " << b.n << ", " << cmp
              << ");\n";
        } else {
            o << "    const bool " << v << " = " << cmp << ";\n";
        }
        return Val{v, "true"};
    }
    // math: null if either side is null (zero slot), one rounding per op
    if (nul) o << "    const bool " << v << "_n = " << both_valid(a, b) << ";\n";
    const std::string valid = nul ? v + "_n" : "true";
    if (op == DFMI_OP_DIVIDE) {
        emit_div_checks(act, valid, a, b, ty, ord, "ERRK_DIV_OVERFLOW");
        if (f)
            o << "    " << ct << " " << v << " = dfmi::sse_nan<" << ct << ">((" << a.v << ") / (" << b.v << "), "
              << a.v << ", " << b.v << ");\n";
        else
            o << "    " << ct << " " << v << " = dfmi::idiv<" << ct << ">(" << a.v << ", " << b.v << ");\n";
    } else if (op == DFMI_OP_MODULUS) {  // extension: the Divide arm's shape -- the checks, then the value
        emit_div_checks(act, valid, a, b, ty, ord, "ERRK_REM_OVERFLOW");
        const IrNode& R = p->ir[n.r];
        if (f)  // (a literal divisor too)
            o << "    " << ct << " " << v << " = dfmi::fn_mod<" << ct << ">(" << a.v << ", " << b.v << ");\n";
        else if (R.kind == IR_LIT && g_rem_literal)  // the reciprocal in a literal slot of its own
            o << "    " << ct << " " << v << " = dfmi::irem_lit<" << ct << ">(" << a.v << ", " << b.v << ", A.lits["
              << lit_at(p, i, 1, rem_reciprocal(type_width(ty), is_signed_int(ty), R.bits)) << "]);\n";
        else
            o << "    " << ct << " " << v << " = dfmi::irem<" << ct << ">(" << a.v << ", " << b.v << ");\n";
    } else if (f) {
        o << "    " << ct << " " << v << " = dfmi::sse_nan<" << ct << ">((" << a.v << ") " << math_sym(op) << " ("
          << b.v << "), " << a.v << ", " << b.v << ");\n";
    } else {
        const char* mt = math_type(ty);
        o << "    " << ct << " " << v << " = (" << ct << ")((" << mt << ")(" << a.v << ") " << math_sym(op) << " ("
          << mt << ")(" << b.v << "));\n";
    }
    if (nul) o << "    if (!" << v << "_n) " << v << " = (" << ct << ")0;\n";
    return Val{v, valid};
}

}  // namespace jit
}  // namespace dfmi
