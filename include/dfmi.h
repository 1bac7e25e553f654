/*
 * dfmi.h — C ABI of the MI355X-native Selection + Projection path.
 *
 * This is the drop-in boundary for the only data-parallel path of the reference
 * (ariesdevil/datafusion v0.5.1): expression compilation plus the
 * FilterRelation/ProjectRelation per-batch evaluation in src/execution/.
 * Every entry point names the reference interface it replaces (file:line under
 * the reference tree). No torch or HIP types appear in the signatures: device
 * buffers are plain pointers, streams are opaque `void*` (hipStream_t).
 *
 * Semantics follow the reference bit-for-bit (see DESIGN.md "Semantics"):
 *   - comparisons never produce nulls; null ordering is arrow 0.12's bool_op
 *     (NULL < x is true, NULL = NULL is true, ...);
 *   - math propagates nulls, Float64 rounds once per operator (no FMA);
 *   - a non-null zero divisor is ArrowError(DivideByZero);
 *   - a Selection drops validity and copies raw slot bits of selected rows;
 *   - only Float64 and Utf8 columns can be filtered unless an extension flag
 *     is given (filter.rs:106-110).
 */
#ifndef DFMI_H
#define DFMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's structs and entry points. 2: dfmi_column.offset
 * (arrow ArrayData::offset), dfmi_abi_version(), the caller-owned output form
 * dfmi_filter_project_host_batches_into. 4: dfmi_sort_batches
 * (DFMI_FLAG_EXT_SORT). Still 4 with DFMI_FLAG_EXT_SCALAR_FUNCTIONS: the
 * change is additive (one flag bit, one new function, no struct change), so
 * a version-4 binding keeps working. A binding compares the library's
 * dfmi_abi_version() with the constant it was built against. */
#define DFMI_ABI_VERSION 4

/* DFMI_ABI_VERSION of the loaded library. */
int32_t dfmi_abi_version(void);

/* ---------------------------------------------------------------------------
 * Types. Subset of arrow::datatypes::DataType that logicalplan.rs can name
 * (ScalarValue logicalplan.rs:93-108, get_supertype logicalplan.rs:443-551).
 * ------------------------------------------------------------------------- */
typedef enum dfmi_type {
    DFMI_TYPE_NULL = 0, /* ScalarValue::Null only */
    DFMI_TYPE_BOOLEAN = 1,
    DFMI_TYPE_INT8 = 2,
    DFMI_TYPE_INT16 = 3,
    DFMI_TYPE_INT32 = 4,
    DFMI_TYPE_INT64 = 5,
    DFMI_TYPE_UINT8 = 6,
    DFMI_TYPE_UINT16 = 7,
    DFMI_TYPE_UINT32 = 8,
    DFMI_TYPE_UINT64 = 9,
    DFMI_TYPE_FLOAT32 = 10,
    DFMI_TYPE_FLOAT64 = 11,
    DFMI_TYPE_UTF8 = 12
} dfmi_type;

/* Status codes: ExecutionError variants (error.rs:27-35) plus the ArrowError
 * kinds array_ops can raise, plus Rust panics and ABI failures. */
typedef enum dfmi_status {
    DFMI_OK = 0,
    DFMI_ERR_EXECUTION = 1,       /* ExecutionError::ExecutionError(String) */
    DFMI_ERR_GENERAL = 2,         /* ExecutionError::General(String) */
    DFMI_ERR_INVALID_COLUMN = 3,  /* ExecutionError::InvalidColumn(String) */
    DFMI_ERR_NOT_IMPLEMENTED = 4, /* ExecutionError::NotImplemented(String) */
    DFMI_ERR_DIVIDE_BY_ZERO = 5,  /* ExecutionError::ArrowError(DivideByZero) */
    DFMI_ERR_ARROW_COMPUTE = 6,   /* ExecutionError::ArrowError(ComputeError) */
    DFMI_ERR_PANIC = 7,           /* the reference panics (unwrap / i64 overflow) */
    DFMI_ERR_INVALID_ARGUMENT = 8,/* ABI misuse (bad pointer, alignment, sizes) */
    DFMI_ERR_CAPACITY = 9,        /* caller-provided output buffer too small */
    DFMI_ERR_DEVICE = 10,         /* HIP runtime failure / device timeout */
    DFMI_ERR_ARROW_PARSE = 11     /* ExecutionError::ArrowError(ParseError): CSV field */
} dfmi_status;

typedef struct dfmi_error {
    int32_t code;       /* dfmi_status */
    char message[500];  /* the reference's message text for that error */
} dfmi_error;

/* ---------------------------------------------------------------------------
 * Columnar batch (Arrow 0.12 memory layout, arrow::record_batch::RecordBatch).
 *   fixed width: `values` holds length * width bytes, native little-endian;
 *   Boolean: `values` is an LSB-first bitmap;
 *   Utf8 (BinaryArray): `offsets` holds length+1 int32, `values` the bytes.
 * `validity` is an LSB-first bitmap, NULL when the column has no nulls.
 * Bitmaps and values must be 8-byte aligned; device pointers for execution.
 * ------------------------------------------------------------------------- */
typedef struct dfmi_column {
    int32_t type;            /* dfmi_type */
    int32_t reserved;
    int64_t length;          /* rows */
    int64_t null_count;
    const uint8_t* validity; /* NULL => all valid */
    const void* values;
    const int32_t* offsets;  /* Utf8 only */
    /* arrow 0.12 ArrayData::offset (a sliced array): logical row i is physical
     * slot offset + i -- values[offset + i], validity / Boolean bit offset + i,
     * Utf8 offsets[offset + i] -- as value(i) / is_null(i) read it
     * (filter.rs:88-89,99-100). 0 for an unsliced array. */
    int64_t offset;
} dfmi_column;

typedef struct dfmi_batch {
    int32_t num_columns;
    int32_t reserved;
    int64_t num_rows;
    const dfmi_column* columns;
} dfmi_batch;

typedef struct dfmi_field {     /* arrow::datatypes::Field */
    const char* name;
    int32_t type;               /* dfmi_type */
    int32_t nullable;
} dfmi_field;

typedef struct dfmi_schema {    /* arrow::datatypes::Schema */
    int32_t num_fields;
    int32_t reserved;
    const dfmi_field* fields;
} dfmi_schema;

/* ---------------------------------------------------------------------------
 * Expressions: logicalplan::Expr (logicalplan.rs:133-164) flattened to
 * postfix order (children first, left before right), i.e. the order in which
 * compile_scalar_expr (expression.rs:244) evaluates them.
 * ------------------------------------------------------------------------- */
typedef enum dfmi_expr_kind {
    DFMI_EXPR_COLUMN = 1,             /* Expr::Column(index) */
    DFMI_EXPR_LITERAL = 2,            /* Expr::Literal(ScalarValue) */
    DFMI_EXPR_BINARY = 3,             /* Expr::BinaryExpr{left, op, right} */
    DFMI_EXPR_CAST = 4,               /* Expr::Cast{expr, data_type} */
    DFMI_EXPR_IS_NULL = 5,            /* Expr::IsNull */
    DFMI_EXPR_IS_NOT_NULL = 6,        /* Expr::IsNotNull */
    DFMI_EXPR_SORT = 7,               /* Expr::Sort */
    DFMI_EXPR_SCALAR_FUNCTION = 8,    /* Expr::ScalarFunction */
    DFMI_EXPR_AGGREGATE_FUNCTION = 9  /* Expr::AggregateFunction */
} dfmi_expr_kind;

typedef enum dfmi_operator {          /* logicalplan::Operator (logicalplan.rs:67-81) */
    DFMI_OP_EQ = 0,
    DFMI_OP_NOT_EQ = 1,
    DFMI_OP_LT = 2,
    DFMI_OP_LT_EQ = 3,
    DFMI_OP_GT = 4,
    DFMI_OP_GT_EQ = 5,
    DFMI_OP_PLUS = 6,
    DFMI_OP_MINUS = 7,
    DFMI_OP_MULTIPLY = 8,
    DFMI_OP_DIVIDE = 9,
    DFMI_OP_MODULUS = 10,
    DFMI_OP_AND = 11,
    DFMI_OP_OR = 12
} dfmi_operator;

typedef struct dfmi_expr_node {
    int32_t kind;       /* dfmi_expr_kind */
    int32_t op;         /* BINARY: dfmi_operator; SORT: asc (1/0) */
    int32_t data_type;  /* LITERAL: ScalarValue variant; CAST/functions: target type */
    int32_t column;     /* COLUMN: index; functions: argument count */
    int64_t i64;        /* LITERAL Int*, UInt* (bit pattern), Boolean (0/1) */
    double f64;         /* LITERAL Float32/Float64 (Float32 stored widened) */
    const char* str;    /* LITERAL Utf8 bytes; functions: name */
    int64_t str_len;
} dfmi_expr_node;

/* Extension flags. 0 = exactly the reference's behaviour. */
#define DFMI_FLAG_EXT_GATHER_ALL   0x1u /* filter Int64 (and other fixed-width) columns
                                           instead of "filter not supported for ..." */
#define DFMI_FLAG_EXT_UTF8_COMPARE 0x2u /* Utf8 literals and Utf8 =/!= comparisons
                                           instead of "No support for literal type" */
#define DFMI_FLAG_EXT_CAST         0x4u /* CAST(<numeric expression> AS <numeric type>)
                                           instead of "column reference" / "CAST not
                                           implemented for expression" (expression.rs:281-290,
                                           321-324): arrow 0.12 cast kernel rules -- a null
                                           stays null, a value the target type cannot hold
                                           (num::cast -> None: out of range, NaN to an
                                           integer) becomes null. Literal casts stay exactly
                                           the reference's (Int64 -> Float64 only). */
#define DFMI_FLAG_EXT_IS_NULL      0x8u /* IsNull / IsNotNull (expression.rs:326-345,
                                           commented out in the reference): the operand's
                                           validity as a non-null Boolean */

#define DFMI_FLAG_EXT_AGGREGATE    0x10u /* LogicalPlan::Aggregate, with or without GROUP BY
                                           (sqlplanner.rs:91-117, compile_expr
                                           expression.rs:81-116) instead of the
                                           executor's unimplemented!() (context.rs:161):
                                           MIN / MAX / SUM / COUNT over the selected
                                           rows, semantics in DESIGN.md §2 */

#define DFMI_FLAG_EXT_SORT         0x20u /* LogicalPlan::Sort and LogicalPlan::Limit
                                           (sqlplanner.rs:119-163) instead of the executor's
                                           unimplemented!() (context.rs:161): a stable sort
                                           of every input row by the key list and / or the
                                           first n rows, dfmi_sort_batches below, semantics
                                           in DESIGN.md §2 */

#define DFMI_FLAG_EXT_SCALAR_FUNCTIONS 0x40u
/* Expr::ScalarFunction (DFMI_EXPR_SCALAR_FUNCTION; planned by sqlplanner.rs:330-350,
 * executed nowhere in the reference) instead of the compile error
 * "expression NAME(...)": the built-in functions
 *     sqrt abs floor ceil round trunc   (one argument)      mod   (two arguments)
 * with the SQL signature (Float64, ...) -> Float64 that dfmi_scalar_function_meta
 * below reports to the planner. Names are lower-case and matched exactly.
 * The node's `column` is the argument count, `str` the name and `data_type`
 * the return type; the arguments precede it in postfix order. The compiler
 * accepts Float64, or Float32 (every argument and data_type the same one of
 * the two; the Float32 form is computed in Float32).
 * Compile-time errors, all DFMI_ERR_EXECUTION:
 *     Invalid function 'NAME'
 *     Function 'NAME' expects N arguments, got M
 *     Function 'NAME' is not supported for (T1, T2) -> R
 * The program's name is the expression's Debug text, e.g.
 * "sqrt(CAST(#3 AS Float64))". The result is null where any argument is null
 * (value slot zero), and no function raises a run-time error. Values are
 * those of Rust's f64 / f32 methods on x86-64, bit for bit:
 *   sqrt   correctly rounded, subnormals included; sqrt(-0.0) = -0.0; a negative
 *          argument (-inf too) gives the default NaN 0xFFF8000000000000 /
 *          0xFFC00000;
 *   abs    clears the sign bit and nothing else (a NaN keeps its payload and
 *          is not quieted);
 *   floor ceil trunc   exact, a zero result keeps the argument's sign
 *          (ceil(-0.5) = -0.0);
 *   round  half away from zero (round(-0.5) = -1.0, round(-0.4) = -0.0);
 *   mod    C fmod: exact, the sign of x, |result| < |y|. y = +-0 or x = +-inf
 *          is an invalid operation and gives the default NaN -- NOT
 *          DFMI_ERR_DIVIDE_BY_ZERO, which only the Divide operator raises.
 * Except for abs, a NaN argument comes back quieted with sign and payload
 * kept, the left argument's first (the rule of the math operators).
 * Transcendental functions are left out on purpose: their results differ
 * between math libraries. The flag adds one bit and one entry point and
 * changes no struct, so DFMI_ABI_VERSION stays 4. */

#define DFMI_FLAG_EXT_AGG_AVG      0x80u /* with DFMI_FLAG_EXT_AGGREGATE: the aggregate
                                           function `avg` (planned by sqlplanner.rs:296 in
                                           one arm with min / max / sum, executed nowhere
                                           in the reference) instead of the panic
                                           "Unsupported aggregate function 'avg'": the
                                           exact mean rounded once, semantics in the
                                           aggregate section below. One bit and one enum
                                           value, no struct change: DFMI_ABI_VERSION
                                           stays 4 */

#define DFMI_FLAG_EXT_UTF8_ORDER   0x100u
/* With DFMI_FLAG_EXT_UTF8_COMPARE (alone it changes nothing): the ordering
 * operators Lt, LtEq, Gt, GtEq over two Utf8 operands instead of the run-time
 * ExecutionError("comparison_ops"). The planner already builds these plans
 * (get_supertype(Utf8, Utf8) = Utf8); the reference executes no Utf8
 * comparison, so the feature is build-defined, parity unpinned.
 *   operands: column-literal, literal-column, column-column, and
 *             literal-literal (folded when the kernel is generated); mixed
 *             types (Utf8 against Float64, ...) stay "comparison_ops";
 *   result:   a non-null Boolean;
 *   order:    the two byte strings as sequences of unsigned bytes -- the
 *             first differing byte decides, a proper prefix is less (Rust's
 *             [u8] / str order, the GROUP BY / ORDER BY key order). 0x00 and
 *             0x80-0xFF are ordinary bytes, invalid UTF-8 included:
 *             "a" < "a\0", "a\x7f" < "a\x80";
 *   nulls:    as the numeric comparisons (arrow's cmp_opt): never a null
 *             result, a null is less than every value, null against null as
 *             there (Lt / LtEq true, Gt / GtEq false). After a Selection the
 *             columns are all-valid and a null slot compares by its raw
 *             bytes, as Utf8 = does;
 *   errors:   none of its own; its operands' ordinals come before its own;
 *   limits:   8 string literals and 256 literal bytes per kernel, as for =.
 * It runs wherever Utf8 = runs (predicates, Boolean projections, aggregate
 * arguments, GROUP BY / ORDER BY key expressions; every batch form). Without
 * both flags every expression compiles and fails exactly as before. One flag
 * bit, no struct change, no new entry point: DFMI_ABI_VERSION stays 4. */

#define DFMI_FLAG_EXT_AGG_MINMAX_ANY 0x200u
/* With DFMI_FLAG_EXT_AGGREGATE (alone it changes nothing): `min` / `max`
 * (any letter case) over a Boolean or Utf8 argument instead of
 * DFMI_ERR_NOT_IMPLEMENTED "aggregate over Boolean" / "aggregate over Utf8";
 * return_type = the argument's type. The planner builds the plan
 * (sqlplanner.rs:296-303) and the reference's aggregate fixtures expect it;
 * nothing in the reference runs it, so the feature is build-defined, parity
 * pinned only by those fixture cells.
 *   rows:     a row counts exactly when COUNT(e) counts it on the same path:
 *             valid slots only, and after a Selection (no validity,
 *             filter.rs:84-93) a selected null slot counts with its raw bit /
 *             slot bytes; dfmi_agg_value.count is that count, and the result
 *             is null when no row counts;
 *   Boolean:  false < true; type Boolean, bits 0 / 1. Its partial is an
 *             integer MIN / MAX partial over 0 / 1 -- the wire format is
 *             unchanged and every merge / shard entry point takes it -- and it
 *             runs everywhere numeric MIN / MAX runs (ungrouped, key window,
 *             hash table, every batch form, host merge, device finish);
 *   Utf8:     the GROUP BY / ORDER BY / DFMI_FLAG_EXT_UTF8_ORDER order:
 *             sequences of unsigned bytes, the first differing byte decides, a
 *             proper prefix is less; 0x00 and 0x80-0xFF are ordinary bytes;
 *             the empty string is the least value and not null. type Utf8,
 *             bits = the value's byte length (0 for null); the bytes come from
 *             dfmi_agg_state_value_bytes. The result does not depend on row
 *             order, batch size or path. The argument must be something the
 *             evaluation pass produces for COUNT(e) (in practice a column).
 *             Ungrouped states and grouped states of 1 to 4 keys of any type,
 *             every batch form, further batches after a finish, reset;
 *   partials: of a state or a merge with a Utf8 MIN / MAX: the wire format
 *             carries no string -- dfmi_agg_state_partial,
 *             dfmi_agg_state_grouped_partial(_bytes), dfmi_shard_agg_finish*,
 *             dfmi_agg_merge_partials and dfmi_agg_merge_grouped_partials*
 *             return DFMI_ERR_NOT_IMPLEMENTED "partial state of a Utf8 MIN /
 *             MAX aggregate".
 * `sum` / `avg` over Boolean / Utf8 keep their errors. Without both flags
 * every call compiles, runs and fails as before. One flag bit and one entry
 * point, no struct change: DFMI_ABI_VERSION stays 4. */

#define DFMI_FLAG_EXT_MODULUS      0x400u
/* Operator::Modulus (DFMI_OP_MODULUS, SQL `%`; planned by sqlplanner.rs:263,
 * executed nowhere in the reference) instead of the compile error
 * ExecutionError("operator: Modulus"). Without the flag -- whatever other
 * flags are set -- that error stays exactly as it is, and the generated code
 * of an expression without a Modulus node does not change with the flag.
 * Beyond the reference's two fixtures (numerics_modulo*.csv) the feature is
 * build-defined, parity unpinned.
 *   types:    as Plus / Minus / Multiply / Divide (math_ops!): the result has
 *             the left operand's type; both operands must have the same type,
 *             one of Int8..Int64, UInt8..UInt64, Float32, Float64. Anything
 *             else (Int64 % Float64, Utf8, Boolean) compiles and carries the
 *             run-time ExecutionError("math_ops") at the node's ordinal, as
 *             for the other four. The name is "<l> Modulus <r>";
 *   nulls:    null (value slot zero) where either side is null; a null row
 *             raises nothing;
 *   integers: Rust's `%`: the truncated remainder with the sign of the
 *             dividend (-7 % 3 = -1, 7 % -3 = 1), computed in the operand's
 *             width. For non-null operands of a selected row, and only
 *             those: a zero divisor is DFMI_ERR_DIVIDE_BY_ZERO
 *             "DivideByZero" (the rule of Divide), and iN::MIN % -1 is Rust's
 *             panic, DFMI_ERR_PANIC "attempt to calculate the remainder with
 *             overflow";
 *   floats:   Rust's f64 % / f32 % on x86-64 (C fmod: exact, the sign of the
 *             dividend, |result| < |divisor|), in the operand's width. A
 *             non-null +-0.0 divisor is DFMI_ERR_DIVIDE_BY_ZERO, checked
 *             before any NaN rule, as for Divide. Otherwise a NaN operand
 *             comes back quieted (the left one first) and an infinite
 *             dividend gives the default NaN. THE DIFFERENCE to the scalar
 *             function mod(x, y) (DFMI_FLAG_EXT_SCALAR_FUNCTIONS) is the zero
 *             divisor alone: mod() returns the default NaN and raises nothing,
 *             the operator raises DivideByZero; every other value is the same;
 *   errors:   the operands' ordinals come before the node's own, and the
 *             first error by (ordinal, row) is the one reported, so sharded,
 *             chunked and coalesced runs report what one pass would;
 *   where:    wherever Divide runs -- predicates, projections, aggregate
 *             arguments, GROUP BY / ORDER BY key expressions; every batch form.
 * A literal divisor (`col % 10`) is reduced by a reciprocal the host computes
 * per launch and passes in a literal slot of its own (32 slots per kernel;
 * DFMI_ERR_NOT_IMPLEMENTED "query compiler: too many literals" past that); the
 * values and errors are those of the general form. One flag bit, no struct
 * change, no new entry point: DFMI_ABI_VERSION stays 4. */

#define DFMI_FLAG_EXT_CAST_ANY     0x800u
/* The rest of CAST, effective only together with DFMI_FLAG_EXT_CAST (as
 * UTF8_ORDER is with UTF8_COMPARE): without both flags every expression
 * compiles and fails exactly as before, and the generated code of a shape
 * without such a cast does not change with the flag. Build-defined, parity
 * unpinned: the reference executes no CAST of a column.
 *   forms:    CAST(e AS T), e not a literal, where (a) e is a Utf8 COLUMN and T
 *             is Boolean, Int8..Int64, UInt8..UInt64, Float32 or Float64; or
 *             (b) e is Boolean and T numeric; or (c) e is numeric and T
 *             Boolean. The name is "CAST(#i AS Type)" as for the numeric casts.
 *             Left out, with their NotImplemented("CAST from .. to ..") text
 *             unchanged: T = Utf8 (numeric -> Utf8 needs computed Utf8 outputs
 *             and shortest float formatting), Utf8 -> Utf8, a Utf8 literal
 *             child; Boolean = / < comparisons stay comparison_ops errors;
 *   nulls:    arrow's cast rule, as for the numeric casts: a null input gives
 *             a null, a value the target cannot hold -- a string that does not
 *             parse -- becomes a null with value slot zero; no cast raises an
 *             error but the one program limit below. After a Selection the
 *             columns are all-valid and a null slot is parsed by its raw bytes
 *             (the rule of Utf8 `=`), in practice "", which is a null;
 *   Boolean:  true -> 1, false -> 0 (1.0 / 0.0); numeric -> Boolean is x != 0,
 *             so NaN is true and -0.0 false, never null for a valid input;
 *   strings:  a cast of a string gives what the native CSV reader
 *             (dfmi_csv_*) gives for a field with that text -- Rust's
 *             str::parse -- and a null where the reader reports a parse error:
 *             integers: [+-] (a '-' only for signed targets: "-0" to an
 *               unsigned type is null), then ASCII digits only, at least one;
 *               no blanks, '.', exponent, '_', non-ASCII digits; a NUL byte is
 *               a wrong byte; any number of leading zeros; out of range: null;
 *             Boolean: "true" / "false" in any ASCII letter case;
 *             floats: [+-], then inf / infinity / nan in any case, or digits
 *               with an optional '.' (at least one digit overall) and an
 *               optional e|E [+-] digits (any length, saturating). nan is the
 *               positive quiet NaN (0x7FF8.. / 0x7FC00000), -nan its negation.
 *               Otherwise the decimal value correctly rounded (nearest, ties
 *               to even) directly to the target width -- Float32 is not
 *               rounded through Float64 -- subnormals at their quantum, +-inf
 *               beyond the range (not null), +-0 with the sign kept below half
 *               the least subnormal;
 *   limit:    the digit string without its leading zeros is read through its
 *             first 19 digits (the most that always fit 64 bits); later digits
 *             only count as "some dropped digit is nonzero". If none is, the
 *             value is exact. Otherwise it lies strictly between w * 10^e and
 *             (w + 1) * 10^e: where both round to one float, that is the
 *             result; where they differ the row raises
 *             DFMI_ERR_NOT_IMPLEMENTED "device program limit: CAST to Float64
 *             needs more than 19 significant digits" ("Float32" likewise) at
 *             the node's ordinal, for evaluated non-null rows only, the first
 *             error by (ordinal, row) winning as for Divide. Machine-written
 *             floats have at most 17 digits and never reach it;
 *   where:    wherever a numeric CAST runs -- predicates, projections,
 *             aggregate arguments, GROUP BY / ORDER BY key expressions; every
 *             batch form; sliced arrays.
 * One flag bit, no struct change, no new entry point: DFMI_ABI_VERSION stays 4. */

#define DFMI_FLAG_EXT_CAST_UTF8    0x1000u
/* CAST to Utf8: numbers and Booleans formatted on the device. Effective only
 * together with DFMI_FLAG_EXT_CAST; without both flags everything compiles and
 * fails exactly as before (dfmi_compile_scalar_expr answers
 * NotImplemented("CAST from Int64 to Utf8") and so on). Build-defined, parity
 * unpinned: the reference executes no CAST of a column. The convention is
 * "what Rust on x86-64 prints" (to_string / Display), so the native CSV reader
 * (dfmi_csv_*) and CAST(s AS T) under DFMI_FLAG_EXT_CAST_ANY read every output
 * back to the value it came from.
 *   forms:    CAST(e AS Utf8) as the ROOT of a projection expression (also a
 *             non-Column ORDER BY key, which is evaluated as a projection),
 *             e of type Boolean, Int8..Int64, UInt8..UInt64, Float32 or
 *             Float64, or a Utf8 COLUMN (identity: the column itself). Name
 *             "CAST(#i AS Utf8)", type Utf8. The fused pass
 *             (dfmi_filter_project*) is not changed: a binding compiles and
 *             runs the cast's CHILD as an ordinary fixed-width projection and
 *             hands the resulting device column to dfmi_format_utf8_batches
 *             below. dfmi_compile_scalar_expr itself keeps its error for every
 *             cast to Utf8, so one anywhere else -- under a comparison, as an
 *             aggregate argument, as a GROUP BY key, with a Utf8 literal child
 *             -- fails with today's text;
 *   nulls:    a null stays a null: an empty slot, the validity copied from the
 *             child's. Nothing raises at run time but the one program limit
 *             below. After a Selection the child column is all-valid and a null
 *             slot is formatted by its raw bits (the rule of Utf8 `=`);
 *   Boolean:  "true" / "false";
 *   integers: ASCII digits without leading zeros, a leading '-' for negative
 *             values: i64::MIN is "-9223372036854775808" (20 bytes), u64::MAX
 *             "18446744073709551615" (20 bytes);
 *   floats:   never exponent notation. The digits are the SHORTEST decimal
 *             digit string that reads back to the same float in the value's
 *             own width (Float32 is not widened: 0.1f32 is "0.1"); of several
 *             shortest strings the one closest to the value, a tie between two
 *             going to the even last digit; an end of the rounding interval
 *             counts as inside when the significand is even (it reads back by
 *             ties-to-even) -- what Rust's Grisu with its Dragon fallback, Ryu,
 *             CPython's repr and std::to_chars produce. The digits are laid out
 *             positionally: "1", "0.1", "1000000000000000000000" for 1e21,
 *             "100000000000000000000000" for 1e23 (the shortest digits, then
 *             zeros: not the float's exact integer value), "0.000..005" for
 *             5e-324. An integral value has no ".0". -0.0 is "-0" (current Rust
 *             prints it so, and the sign survives the round trip). Infinities
 *             are "inf" / "-inf"; every NaN is "NaN", sign and payload dropped
 *             (it reads back as the positive quiet NaN). The longest Float64
 *             string is 327 bytes ("-0." 323 zeros "5" for -5e-324), the
 *             longest Float32 string 48 bytes (-1e-45);
 *   limit:    a column of 2^31 or more output bytes is DFMI_ERR_NOT_IMPLEMENTED
 *             "device program limit: CAST to Utf8 output of 2^31 or more bytes".
 * One flag bit, one new entry point, no struct change: DFMI_ABI_VERSION stays 4. */

#define DFMI_FLAG_EXT_CSV_WRITE    0x2000u
/* CSV output: PhysicalPlan::Write { plan, filename, kind } (physicalplan.rs:24-29,
 * "Execute a logical plan and write the output to a file"), which the reference
 * defines and never runs. Result batches are encoded as CSV on the device by
 * dfmi_csv_encode_batches below; dfmi_csv_header gives the header line.
 * Build-defined, parity unpinned: arrow 0.12 has no CSV writer. The dialect is
 * "what the native CSV reader (include/dfmi_datasource.h) and the reference's
 * CsvDataSource read back to the same values":
 *   records:  one per row, in row order and batch order; fields separated by
 *             ','; every record ends with '\n', the last one too; no '\r' is
 *             ever written as a line end;
 *   Boolean, integers, floats: exactly the bytes of CAST(e AS Utf8) under
 *             DFMI_FLAG_EXT_CAST_UTF8 above -- "true" / "false"; digits with a
 *             leading '-'; the shortest digits that read back in the value's own
 *             width, never an exponent; "-0", "inf", "-inf", "NaN";
 *   null:     a null of any type is an empty field. A Utf8 null and the empty
 *             string are the same bytes (the reader gives "" for both);
 *   Utf8:     the bytes as they are. The field is quoted exactly when it holds
 *             '"', ',', '\n' or '\r'; inside quotes a '"' is doubled. 0x00 and
 *             0x80-0xFF are ordinary bytes; a space never forces quotes;
 *   empty record: a record of ONE column whose only field is empty (a null, an
 *             empty string) is written as `""`: the reader skips empty records,
 *             reads `""` as the empty string and, in a numeric column, as null;
 *   no validity: a column without validity (every batch after a Selection) has
 *             no nulls: a slot is formatted from its raw bits -- the rule of
 *             Utf8 `=` and of CAST to Utf8;
 *   header:   the field names joined by ',' and ended by '\n', under the same
 *             quoting rule (and the same one-column rule).
 * One flag bit, two new entry points, no struct change: DFMI_ABI_VERSION stays 4. */

/* Signature of a built-in scalar function, for a binding's
 * SchemaProvider::get_function_meta (sqlplanner.rs:330-350 casts each
 * argument to arg_types[i]). Returns 0 and fills *num_args, *return_type and
 * the first min(*num_args, max_args) entries of arg_types (dfmi_type values)
 * for a known name; nonzero, with nothing written, for an unknown one (the
 * planner then raises its own "Invalid function 'NAME'"). NULL outputs are
 * skipped. Needs no context and no flag: it only reads the table. */
int32_t dfmi_scalar_function_meta(const char* name, int32_t name_len, int32_t* arg_types,
                                  int32_t max_args, int32_t* num_args, int32_t* return_type);

/* Opaque compiled expression: the RuntimeExpr::Compiled of expression.rs:43-50. */
typedef struct dfmi_program dfmi_program;

/* compile_scalar_expr (expression.rs:244-451). Rejects exactly what the
 * reference rejects at compile time, with the same error variant and text.
 * Errors the reference raises only when the closure runs (comparison_ops,
 * math_ops, panics) are recorded in the program and reported by execution. */
int32_t dfmi_compile_scalar_expr(const dfmi_expr_node* nodes, int32_t num_nodes,
                                 const dfmi_schema* input_schema, uint32_t flags,
                                 dfmi_program** out, dfmi_error* err);

/* RuntimeExpr::get_name / get_type (expression.rs:64-77). */
const char* dfmi_program_name(const dfmi_program* program);
int32_t dfmi_program_type(const dfmi_program* program);
void dfmi_program_free(dfmi_program* program);

/* ---------------------------------------------------------------------------
 * Execution context: one per (GPU, stream). Holds the look-back tile-status
 * workspace, result counters and error words. Not thread-safe; one host
 * thread per context (the reference is single-threaded, context.rs:33).
 * ------------------------------------------------------------------------- */
typedef struct dfmi_context dfmi_context;

int32_t dfmi_context_create(int32_t device, void* hip_stream, dfmi_context** out,
                            dfmi_error* err);
void dfmi_context_destroy(dfmi_context* ctx);
/* Rebind the stream used by later calls (e.g. torch's current stream). */
int32_t dfmi_context_set_stream(dfmi_context* ctx, void* hip_stream);

/* Output column. The caller provides device buffers sized for the worst case:
 *   values:   num_rows * width bytes (Boolean: ceil(num_rows/8), 8-padded);
 *   validity: ceil(num_rows/8) bytes, 8-padded; written when the result can
 *             hold nulls (always without a predicate; after a Selection only
 *             for a projection with a fallible CAST, DFMI_FLAG_EXT_CAST) --
 *             null_count > 0 says it holds the result's validity;
 *   offsets:  (num_rows+1) int32 for Utf8;
 *   data:     Utf8 bytes, data_capacity >= input column's byte length.
 * The library fills the fields below the line. */
typedef struct dfmi_out_column {
    void* values;
    uint8_t* validity;
    int32_t* offsets;
    uint8_t* data;
    int64_t data_capacity;
    /* ---- filled by dfmi_filter_project ---- */
    int32_t type;                /* dfmi_type of the result array */
    int32_t passthrough_column;  /* >=0: result IS that input column (Arc clone,
                                    expression.rs:272-276); buffers untouched */
    int64_t length;
    int64_t null_count;          /* 0 => validity not written / not needed */
    int64_t data_length;         /* Utf8 bytes written */
} dfmi_out_column;

/* One pull of ProjectRelation::next(FilterRelation::next(batch))
 * (projection.rs:45-66, filter.rs:46-72, filter() filter.rs:80-111),
 * fused into one pass over HBM.
 *   predicate == NULL       : no Selection in the plan (projection only);
 *   num_projections == 0    : no Projection: FilterRelation output = every
 *                             input column filtered (outputs has num_columns);
 * The call is synchronous: on return `outputs[i].length` is the batch's row
 * count. Errors are the ones the reference's next() returns. */
int32_t dfmi_filter_project(dfmi_context* ctx, const dfmi_program* predicate,
                            const dfmi_program* const* projections, int32_t num_projections,
                            const dfmi_batch* input, dfmi_out_column* outputs,
                            uint32_t flags, dfmi_error* err);

/* ---------------------------------------------------------------------------
 * Coalesced form for small batches: the pull of dfmi_filter_project on each
 * of `num_batches` device batches IN ORDER, as the reference's pull loop
 * runs them one next() at a time (csv_sql.rs:49 reads 1024-row batches and
 * pulls them in csv_sql.rs:60-62; relation.rs:27-32), but as ONE kernel
 * launch for all of them. Batches share the schema (column types); each has
 * its own rows, buffers and outputs: `outputs` holds num_batches x n
 * columns, batch-major (n = num_projections, or num_columns without a
 * projection), each sized for its own batch as in dfmi_filter_project. Every
 * batch gets exactly the output dfmi_filter_project would give it (one
 * output batch per input batch, 0-row batches included).
 * Errors: the call returns the error of the first batch that raises one;
 * *failed_batch names it and the batches before it are complete -- the
 * caller hands those out first, as the pull loop would have seen them. A
 * plan error the reference raises on every batch fails batch 0.
 * ------------------------------------------------------------------------- */
int32_t dfmi_filter_project_batches(dfmi_context* ctx, const dfmi_program* predicate,
                                    const dfmi_program* const* projections, int32_t num_projections,
                                    const dfmi_batch* inputs, int32_t num_batches, dfmi_out_column* outputs,
                                    uint32_t flags, int32_t* failed_batch, dfmi_error* err);

/* ---------------------------------------------------------------------------
 * Host-buffer form, for callers whose batches live in host memory (the Rust
 * reference's arrow 0.12 buffers from csv::Reader, csv_sql.rs:49): the same
 * pull as dfmi_filter_project -- FilterRelation::next (filter.rs:46-72) +
 * filter() (filter.rs:80-111) + ProjectRelation::next (projection.rs:45-66)
 * -- but `input` holds HOST pointers. Rows are independent, so the library
 * cuts the batch into row chunks (~48 MiB of input each) and pipelines them:
 * host staging copies, H2D DMA, the fused pass and D2H DMA of consecutive
 * chunks overlap; chunk results are concatenated in row order into host
 * buffers the library owns until dfmi_host_result_free. The result and any
 * error are those of one pull over the whole batch (the first error in the
 * reference's evaluation order over all rows). Passthrough columns (Arc
 * clones, expression.rs:272-276) are returned as copies.
 * ------------------------------------------------------------------------- */
typedef struct dfmi_host_result dfmi_host_result;

int32_t dfmi_filter_project_host(dfmi_context* ctx, const dfmi_program* predicate,
                                 const dfmi_program* const* projections, int32_t num_projections,
                                 const dfmi_batch* input, uint32_t flags,
                                 dfmi_host_result** out, dfmi_error* err);
int32_t dfmi_host_result_num_columns(const dfmi_host_result* result);
/* Host view of result column i; buffers stay valid until the result is freed.
 * `validity` is NULL when null_count == 0 (filtered outputs never have one). */
int32_t dfmi_host_result_column(const dfmi_host_result* result, int32_t i, dfmi_column* view);
/* Views of columns [first, first + count) in one call (views[k] as
 * dfmi_host_result_column(first + k)): a binding that hands out one output
 * batch per input batch of the coalesced form below reads every batch's
 * views at once instead of one FFI call per column. */
int32_t dfmi_host_result_columns(const dfmi_host_result* result, int32_t first, int32_t count, dfmi_column* views);
/* The one pinned block holding the columns of a coalesced result (NULL / 0
 * for the single-batch pipelined form): a binding may wrap it once and slice
 * every column's buffers out of it, keeping the result alive while any such
 * slice is. Passthrough columns live outside it. */
int32_t dfmi_host_result_block(const dfmi_host_result* result, const void** base, size_t* bytes);
void dfmi_host_result_free(dfmi_host_result* result);

/* Coalesced form of dfmi_filter_project_host for many small HOST batches
 * (csv_sql.rs:49-62: 1024-row batches read from csv::Reader, pulled one
 * next() at a time): the batches' buffers are packed into pinned memory, moved
 * with one H2D copy, run as one dfmi_filter_project_batches launch, and the
 * outputs come back with one D2H copy. The result holds num_batches x n
 * columns, batch-major (n = num_projections, or num_columns without a
 * projection). Errors as dfmi_filter_project_batches: the call returns the
 * error of the first batch that raises one and *failed_batch names it; the
 * result is still returned, with the batches before it complete and the rest
 * empty (the caller hands those out first). Free the result in every case. */
int32_t dfmi_filter_project_host_batches(dfmi_context* ctx, const dfmi_program* predicate,
                                         const dfmi_program* const* projections, int32_t num_projections,
                                         const dfmi_batch* inputs, int32_t num_batches, uint32_t flags,
                                         dfmi_host_result** out, int32_t* failed_batch, dfmi_error* err);

/* Caller-owned form of dfmi_filter_project_host_batches: the outputs are
 * written into ONE host block the caller allocated (e.g. an arrow 0.12
 * MutableBuffer, which freezes into the Buffer every output array slices --
 * projection.rs:59-60 / filter.rs:60-61 return freshly built arrays per pull),
 * instead of a library-owned result. dfmi_host_batches_output_bytes gives the
 * block's worst-case size for these batches (every row selected); the block
 * must be 64-byte aligned. Each output buffer starts at a 256-byte multiple
 * of the block. `outputs` (num_batches x n, batch-major, n = num_projections
 * or num_columns without a projection) is filled by the library: values /
 * validity (null_count > 0) / Utf8 offsets + data point into the block;
 * passthrough_column >= 0 marks an output that IS that input column (the Arc
 * clone of expression.rs:272-276: the caller reuses its own input array).
 * A block in pinned memory (dfmi_host_alloc, dfmi_host_register, any
 * hipHostMalloc'd allocation) is written by the kernel in place; a pageable
 * block receives the selected bytes with one host copy from the library's
 * pinned staging. Errors and *failed_batch as dfmi_filter_project_host_batches
 * (the batches before the failing one are complete);
 * out_capacity < the size needed -> DFMI_ERR_CAPACITY, nothing run. */
int32_t dfmi_host_batches_output_bytes(const dfmi_program* predicate, const dfmi_program* const* projections,
                                       int32_t num_projections, const dfmi_batch* inputs, int32_t num_batches,
                                       uint32_t flags, size_t* bytes, dfmi_error* err);
int32_t dfmi_filter_project_host_batches_into(dfmi_context* ctx, const dfmi_program* predicate,
                                              const dfmi_program* const* projections, int32_t num_projections,
                                              const dfmi_batch* inputs, int32_t num_batches, uint32_t flags,
                                              void* out_block, size_t out_capacity, dfmi_out_column* outputs,
                                              int32_t* failed_batch, dfmi_error* err);

/* Pinned host memory for batch buffers (e.g. a CSV reader parsing straight
 * into them; csv_sql.rs:49's DataSource side). Columns whose buffers lie in
 * such memory -- or in any hipHostMalloc'd allocation of at least 1 MiB --
 * are DMA'd by dfmi_filter_project_host straight from the caller's memory
 * instead of through the library's pinned staging. dfmi_host_register pins
 * an existing range (hipHostRegister) until dfmi_host_unregister. */
int32_t dfmi_host_alloc(size_t bytes, void** out, dfmi_error* err);
int32_t dfmi_host_free(void* ptr);
int32_t dfmi_host_register(void* ptr, size_t bytes, dfmi_error* err);
int32_t dfmi_host_unregister(void* ptr);

/* The context's GPU is shared with other processes (several ranks on one
 * device, a time-sliced GPU): kernels with a decoupled look-back take their
 * tiles from an atomic ticket counter from the first launch, so a tile never
 * waits on a predecessor another process keeps off the CUs.
 * Default: off, or DFMI_SHARED=1 in the environment at dfmi_context_create.
 * Without it a shared launch still completes, after a 2 s look-back timeout
 * and a ticket-ordered relaunch. */
int32_t dfmi_context_set_shared(dfmi_context* ctx, int32_t shared);

/* HIP events around each launch (default on): dfmi_last_timing needs them;
 * off saves two event records per call on the small-batch path. */
int32_t dfmi_context_set_timing(dfmi_context* ctx, int32_t enable);

/* Device time in milliseconds of the last dfmi_filter_project's kernels
 * (HIP events on the context stream), and the dominant kernel's share. */
int32_t dfmi_last_timing(const dfmi_context* ctx, double* total_ms, double* main_kernel_ms);

/* hipRTC compile time in milliseconds of the last dfmi_filter_project call
 * (0 when its query shape was already compiled: the kernel cache is keyed by
 * the programs and the batch's column types / nullability). */
int32_t dfmi_last_compile_ms(const dfmi_context* ctx, double* compile_ms);

/* Name of the query kernel the last dfmi_filter_project / dfmi_aggregate_batch
 * on ctx launched: dfmi_<filter|project|agg>_<hash of the generated code>, as
 * rocprofv3 reports it ("" before the first launch). Diagnostics. */
const char* dfmi_last_kernel_name(const dfmi_context* ctx);

/* Evaluation-order key of the error the last dfmi_filter_project on ctx
 * returned: (position of the failing operator in the reference's evaluation
 * order) << 44 | row << 4; all ones when it returned no such error. Lets a
 * sharded caller report the error the reference would raise first over the
 * whole table (smallest key position, then the earliest shard). */
int32_t dfmi_last_error_order(const dfmi_context* ctx, uint64_t* key);

/* ---------------------------------------------------------------------------
 * Aggregate extension (DFMI_FLAG_EXT_AGGREGATE). The reference plans
 * `SELECT SUM(e), ... FROM t [WHERE p]` as Aggregate(Selection?(TableScan))
 * (sqlplanner.rs:91-117) and compiles each AggregateFunction with
 * compile_expr (expression.rs:81-116: one argument compiled by
 * compile_scalar_expr, AggregateType Min/Max/Count/Sum), but its executor
 * stops at `unimplemented!()` (context.rs:161). Here the whole pull --
 * FilterRelation::next over every batch plus the aggregation -- is one fused
 * pass per batch (no filtered batch is materialised), accumulated in a
 * device state across batches. Semantics (build-defined, oracle-pinned):
 *   COUNT(e): non-null values of e over the selected rows (UInt64);
 *   SUM(e):   integers wrap in e's type; Float32/Float64 are the exact sum
 *             rounded once (round half to even) -- independent of order,
 *             batch and GPU count; a NaN input or +inf with -inf gives the
 *             canonical quiet NaN, otherwise an infinite input gives that
 *             infinity; an exact zero is -0.0 only if every value is -0.0;
 *   MIN/MAX(e): NaN values are skipped (a set of only NaNs gives the
 *             canonical NaN), -0.0 orders below +0.0;
 *   SUM/MIN/MAX over no non-null value is null.
 *   AVG(e) (DFMI_FLAG_EXT_AGG_AVG together with DFMI_FLAG_EXT_AGGREGATE;
 *             without the flag `avg` panics as in the reference; build-defined,
 *             parity unpinned): e is Float64 or Float32 and the result has e's
 *             type (sqlplanner.rs:301-303). With n the non-null values of e over
 *             the selected rows: count = n; n = 0 gives null; a NaN input or
 *             +inf with -inf gives SUM's canonical quiet NaN, otherwise an
 *             infinite input gives that infinity; otherwise the exact rational
 *             (exact sum) / n rounded half to even ONCE -- Float64: 53 bits,
 *             quantum at least 2^-1074; Float32: 24 bits, quantum at least
 *             2^-149; results in the subnormal range are rounded at the
 *             subnormal quantum (AVG(5e-324, 0.0) = +0.0, a tie to even). It is
 *             not fl(fl(SUM)/n), which rounds twice and overflows:
 *             AVG(1.797e308, 1.797e308) is 1.797e308, and finite inputs never
 *             give an infinity. A nonzero exact sum whose mean rounds to zero
 *             keeps the sum's sign; an exact-zero sum follows SUM's rule (-0.0
 *             only if every value is -0.0). n may be anything in [1, 2^63). Like
 *             SUM it does not depend on row order, batch size or GPU count, and
 *             it runs everywhere SUM does with the same bits; an AVG's partial
 *             is a SUM's partial (no wire format changes) and an AVG takes one
 *             of the four float-SUM slots of a state. An integer argument is
 *             DFMI_ERR_NOT_IMPLEMENTED "AVG over <Type>: cast the argument to
 *             Float64" (the state keeps only a wrapping 64-bit integer sum, so
 *             there is no exact sum to divide): write AVG(CAST(c AS DOUBLE)).
 *             Boolean and Utf8 arguments fail as they do for SUM.
 * GROUP BY (dfmi_agg_state_create_grouped / _multi): one to four key
 * expressions of any type the reference's values take -- Boolean, integer,
 * Float32 / Float64 or Utf8; per group the aggregates above. Groups come out
 * in key order, lexicographic over the key parts, each part ordered false <
 * true, integers numerically, floats by IEEE 754 totalOrder with one group per
 * bit pattern -- -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, as
 * Rust's total_cmp --, Utf8 bytewise, with that part's null last -- for one
 * Boolean key the order of the reference's expected/csv_aggregate_by_c_bool.csv.
 * One Boolean / integer key: a batch whose selected keys lie within 16
 * consecutive values runs the fused grouped kernel. Every other batch (wider
 * integer keys, float or Utf8 keys, several keys) runs the keys and the
 * arguments through the fused Selection + Projection pass, then a device hash
 * table (open addressing, one claim pass and one accumulate pass with the
 * same per-row rules; rows whose key shares its 63-bit hash with another
 * key's are merged on the host) -- any number of groups per batch and
 * overall (up to 2^30 per device).
 * ------------------------------------------------------------------------- */
typedef enum dfmi_agg_fn {       /* AggregateType (expression.rs:33-40) */
    DFMI_AGG_MIN = 0,
    DFMI_AGG_MAX = 1,
    DFMI_AGG_SUM = 2,
    DFMI_AGG_COUNT = 3,
    DFMI_AGG_AVG = 4             /* DFMI_FLAG_EXT_AGG_AVG; not an AggregateType of the reference */
} dfmi_agg_fn;

typedef struct dfmi_agg_value {
    int32_t type;      /* dfmi_type of the result (the AggregateFunction return_type) */
    int32_t is_null;   /* 1: no non-null input value (SUM / MIN / MAX) */
    int64_t count;     /* non-null input values aggregated */
    uint64_t bits;     /* integers sign/zero-extended to 64 bits, Float32 bits in the
                          low 32, Float64 bits */
} dfmi_agg_value;

typedef struct dfmi_aggregate dfmi_aggregate;

/* compile_expr's AggregateFunction arm (expression.rs:81-116): `name` as the
 * SQL text spells it (min / max / sum / count, any case, and avg with
 * DFMI_FLAG_EXT_AGG_AVG; anything else panics in the reference: DFMI_ERR_PANIC), `argument` compiled by
 * dfmi_compile_scalar_expr, `return_type` the planner's (sqlplanner.rs:296-330:
 * the argument's type, UInt64 for count). */
int32_t dfmi_compile_aggregate(const char* name, const dfmi_program* argument, int32_t return_type,
                               uint32_t flags, dfmi_aggregate** out, dfmi_error* err);
const char* dfmi_aggregate_name(const dfmi_aggregate* agg);
int32_t dfmi_aggregate_type(const dfmi_aggregate* agg);
void dfmi_aggregate_free(dfmi_aggregate* agg);

/* Device accumulators of one Aggregate plan on one context. */
typedef struct dfmi_agg_state dfmi_agg_state;

int32_t dfmi_agg_state_create(dfmi_context* ctx, const dfmi_aggregate* const* aggs, int32_t num_aggs,
                              dfmi_agg_state** out, dfmi_error* err);
/* One batch of the aggregate's input (FilterRelation::next when predicate is
 * non-NULL), accumulated on the device; asynchronous on the context stream
 * except for error reporting, which is synchronous like dfmi_filter_project. */
int32_t dfmi_aggregate_batch(dfmi_context* ctx, dfmi_agg_state* state, const dfmi_program* predicate,
                             const dfmi_batch* input, uint32_t flags, dfmi_error* err);
/* Many small batches (the reference's 1024-row Relation::next pulls) in ONE
 * call: the state afterwards is the state after dfmi_aggregate_batch on
 * inputs[0..num_batches) in order, bit for bit, for ungrouped and for grouped
 * states. Ungrouped states and one narrow Boolean / integer key run as one
 * batch-table copy, one launch of the batched aggregate kernel (a coalesced
 * MIN / MAX pre-pass finds one key window for the whole call), one copy of
 * the per-batch headers and one synchronisation. Hash-table states (wide
 * integer, float or several keys) evaluate the keys and arguments of every
 * batch in one launch and run the table's passes once over the call's
 * selected rows. A state whose predicate, keys or arguments read a Utf8
 * column runs the call one batch at a time, with the same results and errors. num_batches == 0 is a no-op; 0-row batches, sliced
 * columns and batches that differ in nullability are allowed; batches must
 * share column types (DFMI_ERR_INVALID_ARGUMENT "batches do not share a
 * schema"). On an error the call returns the error of the first batch, in
 * order, on which dfmi_aggregate_batch would have failed, *failed_batch
 * (may be NULL) names it (-1 otherwise) and the state is failed, as after a
 * failing dfmi_aggregate_batch. */
int32_t dfmi_aggregate_batches(dfmi_context* ctx, dfmi_agg_state* state, const dfmi_program* predicate,
                               const dfmi_batch* inputs, int32_t num_batches, uint32_t flags,
                               int32_t* failed_batch, dfmi_error* err);
/* ... over HOST batches (inputs hold host pointers): the columns the
 * predicate, the keys and the arguments read are packed into pinned staging,
 * moved with one copy and run through the device form; nothing but the
 * per-batch headers comes back. A call whose needed bytes exceed the staging
 * budget (64 MiB) is split at batch boundaries into consecutive sub-calls; a
 * single over-size batch is staged alone. */
int32_t dfmi_aggregate_host_batches(dfmi_context* ctx, dfmi_agg_state* state, const dfmi_program* predicate,
                                    const dfmi_batch* inputs, int32_t num_batches, uint32_t flags,
                                    int32_t* failed_batch, dfmi_error* err);
/* The aggregate values over every batch so far (num_aggs entries). */
int32_t dfmi_agg_state_finish(dfmi_context* ctx, dfmi_agg_state* state, dfmi_agg_value* out,
                              dfmi_error* err);
/* Multi-GPU: the exact partial state (count, flags, min/max key, integer sum,
 * exact float sum digits) as dfmi_agg_partial_bytes() host bytes, and the
 * merge of partials from every shard into final values -- bit-identical to
 * one state over all the shards' rows. */
int64_t dfmi_agg_partial_bytes(const dfmi_agg_state* state);
int32_t dfmi_agg_state_partial(dfmi_context* ctx, dfmi_agg_state* state, void* host_out, dfmi_error* err);
int32_t dfmi_agg_merge_partials(const dfmi_aggregate* const* aggs, int32_t num_aggs,
                                const void* const* partials, int32_t num_partials, dfmi_agg_value* out,
                                dfmi_error* err);
/* GROUP BY extension: LogicalPlan::Aggregate{group_expr: [key]}
 * (sqlplanner.rs:91-117; the reference's executor stops at context.rs:161).
 * `key` compiled by dfmi_compile_scalar_expr over the same schema (Boolean,
 * integer, Float32 / Float64 or Utf8), at most 15 aggregates. Batches go
 * through dfmi_aggregate_batch. */
int32_t dfmi_agg_state_create_grouped(dfmi_context* ctx, const dfmi_program* key, const dfmi_aggregate* const* aggs,
                                      int32_t num_aggs, dfmi_agg_state** out, dfmi_error* err);
/* ... with group_expr = keys[0..num_keys) (1 to 4 expressions, the
 * planner's Vec<Expr>, sqlplanner.rs:97-103), evaluated in that order before
 * the aggregates' arguments (their errors come first, in that order). */
int32_t dfmi_agg_state_create_grouped_multi(dfmi_context* ctx, const dfmi_program* const* keys, int32_t num_keys,
                                            const dfmi_aggregate* const* aggs, int32_t num_aggs, dfmi_agg_state** out,
                                            dfmi_error* err);
/* The state's GROUP BY expressions (0: not a grouped state). */
int32_t dfmi_agg_state_num_keys(const dfmi_agg_state* state);
/* The groups so far, in key order: keys[g * num_keys + p] for key part p
 * (type = the part's type, is_null, bits: Boolean 0/1, integers
 * sign/zero-extended, float bits, Utf8 0 -- the bytes come from
 * dfmi_agg_state_group_keys_utf8_part; count = the group's selected rows) and
 * values[g * num_aggs + j]. *num_groups is set even when it exceeds
 * `capacity` (groups; then DFMI_ERR_INVALID_ARGUMENT and nothing is
 * written). */
int32_t dfmi_agg_state_finish_grouped(dfmi_context* ctx, dfmi_agg_state* state, int64_t capacity, dfmi_agg_value* keys,
                                      dfmi_agg_value* values, int64_t* num_groups, dfmi_error* err);
/* The Utf8 key part `part` of the groups of the last
 * dfmi_agg_state_finish_grouped (or dfmi_shard_agg_finish_grouped), in the
 * same order, as an arrow BinaryArray: offsets[0..num_groups] (from 0) and
 * the bytes (a null key's slot is empty; keys[g * num_keys + part].is_null
 * says which). *data_length is set even when a capacity is too small (then
 * DFMI_ERR_CAPACITY and nothing is written). _utf8: part 0. */
int32_t dfmi_agg_state_group_keys_utf8_part(const dfmi_agg_state* state, int32_t part, int32_t* offsets,
                                            int64_t num_offsets, uint8_t* data, int64_t data_capacity,
                                            int64_t* data_length, dfmi_error* err);
int32_t dfmi_agg_state_group_keys_utf8(const dfmi_agg_state* state, int32_t* offsets, int64_t num_offsets, uint8_t* data,
                                       int64_t data_capacity, int64_t* data_length, dfmi_error* err);
/* DFMI_FLAG_EXT_AGG_MINMAX_ANY: the values of aggregate `agg` (a MIN / MAX
 * over a Utf8 argument) from the state's last dfmi_agg_state_finish (one row)
 * or dfmi_agg_state_finish_grouped (num_groups rows, the same order), as an
 * arrow BinaryArray: offsets from 0, a null value's slot empty (the finish's
 * is_null says which). *data_length is always set; a capacity that is too
 * small gives DFMI_ERR_CAPACITY and nothing is written. `agg` out of range or
 * not a Utf8 MIN / MAX, or no finish yet: DFMI_ERR_INVALID_ARGUMENT. */
int32_t dfmi_agg_state_value_bytes(const dfmi_agg_state* state, int32_t agg, int32_t* offsets, int64_t num_offsets,
                                   uint8_t* data, int64_t data_capacity, int64_t* data_length, dfmi_error* err);
/* Multi-GPU GROUP BY: the exact per-group partial state (every key part --
 * Utf8 bytes included --, the group's selected rows, every aggregate's
 * partial) as host bytes -- size first (negative: -status) -- and the merge
 * of every shard's bytes into the groups one state over all the shards' rows
 * would hold, in key order (output as dfmi_agg_state_finish_grouped; the
 * bytes of a Utf8 key part of the merged groups from
 * dfmi_agg_merge_grouped_partials_keys_utf8, same order). */
int64_t dfmi_agg_state_grouped_partial_bytes(dfmi_context* ctx, dfmi_agg_state* state, dfmi_error* err);
int32_t dfmi_agg_state_grouped_partial(dfmi_context* ctx, dfmi_agg_state* state, void* host_out, int64_t bytes,
                                       dfmi_error* err);
int32_t dfmi_agg_merge_grouped_partials(const dfmi_aggregate* const* aggs, int32_t num_aggs,
                                        const void* const* partials, const int64_t* sizes, int32_t num_partials,
                                        int64_t capacity, dfmi_agg_value* keys, dfmi_agg_value* values,
                                        int64_t* num_groups, dfmi_error* err);
int32_t dfmi_agg_merge_grouped_partials_keys_utf8(const dfmi_aggregate* const* aggs, int32_t num_aggs,
                                                  const void* const* partials, const int64_t* sizes,
                                                  int32_t num_partials, int32_t part, int32_t* offsets,
                                                  int64_t num_offsets, uint8_t* data, int64_t data_capacity,
                                                  int64_t* data_length, dfmi_error* err);
/* Back to the empty state (asynchronous on the context stream): re-running the query. */
int32_t dfmi_agg_state_reset(dfmi_context* ctx, dfmi_agg_state* state, dfmi_error* err);
void dfmi_agg_state_free(dfmi_agg_state* state);

/* ---------------------------------------------------------------------------
 * Sort / Limit extension (DFMI_FLAG_EXT_SORT). The reference plans
 * `SELECT ... ORDER BY e [ASC|DESC], ... LIMIT n` as Limit(Sort(Projection))
 * (sqlplanner.rs:119-163) and its executor stops at `unimplemented!()`
 * (context.rs:161). Build-defined semantics:
 *   order: lexicographic over the key list, each key in the GROUP BY key order
 *     above -- false < true, integers numerically, Float32 / Float64 by IEEE
 *     754 totalOrder with one position per bit pattern, Utf8 bytewise (a
 *     prefix first) -- and a null greater than every value; a descending key
 *     reverses its whole comparison (its nulls first); rows equal on every
 *     key keep their input order (batch order, then row order): the sort is
 *     stable in both directions;
 *   limit: the first `limit` rows of that order (ties by input order); < 0:
 *     none; num_keys = 0: the first `limit` rows of the input as it is.
 * `inputs`: num_batches >= 1 device batches of one schema (0-row batches
 * allowed, sliced columns through dfmi_column.offset), all of which stay on
 * the device; they are not copied into one batch. key_columns[k] indexes the
 * batches' columns, key_asc[k] is 1 (ascending) or 0; at most 8 keys and fewer
 * than 2^31 rows and Utf8 output bytes per column (else
 * DFMI_ERR_NOT_IMPLEMENTED, "device program limit: ..."). `outputs`: one entry
 * per input column, buffers sized by the caller for the total row count as
 * dfmi_out_column says, validity for every column that has nulls in some
 * batch, data_capacity >= the column's total input bytes. The library fills
 * type, length = min(limit, total rows), null_count (exact; validity is
 * written whenever some batch's column has nulls, bits past length in its
 * last 64-bit word zero), data_length and passthrough_column = -1. The value
 * bytes of null slots are unspecified. Synchronous. A missing flag, a key out
 * of range or a NULL buffer is DFMI_ERR_INVALID_ARGUMENT.
 * ------------------------------------------------------------------------- */
int32_t dfmi_sort_batches(dfmi_context* ctx, const dfmi_batch* inputs, int32_t num_batches,
                          const int32_t* key_columns, const int32_t* key_asc, int32_t num_keys,
                          int64_t limit /* < 0: none */, dfmi_out_column* outputs,
                          uint32_t flags, dfmi_error* err);

/* ---------------------------------------------------------------------------
 * CAST to Utf8 (DFMI_FLAG_EXT_CAST with DFMI_FLAG_EXT_CAST_UTF8; the values'
 * text is specified at the flag). Formats `num_columns` device columns, each
 * of Boolean or a fixed-width numeric type, with num_rows[i] = columns[i].length
 * rows (0 allowed, sliced columns through dfmi_column.offset), into arrow Utf8
 * arrays -- all the batches of a coalesced pull in ONE call: the kernels run
 * once over every column together. For each column the library writes
 *   outputs[i].offsets[0..n]  int32, starting at 0 (caller: n + 1 words);
 *   outputs[i].validity       the input's validity, bits past n in the last
 *                             64-bit word zero, when the input has nulls
 *                             (validity != NULL and null_count > 0; caller:
 *                             ceil(n / 64) * 8 bytes, 8-byte aligned); a null
 *                             row's slot is empty;
 *   outputs[i].data           the bytes, data_capacity of them at the most;
 *   data_lengths[i]           the bytes the column needs -- always, also when
 *                             the call fails on a capacity or on the limit;
 * and fills type = Utf8, passthrough_column = -1, length, null_count and
 * data_length. Measure mode: with outputs[i].data == NULL the column's offsets
 * and data_lengths[i] are written and no byte is. A Float64 caller measures,
 * allocates exactly and calls again; for the other types the worst case is
 * small enough to allocate at once. Bytes per row that always suffice:
 *     UInt8 3   UInt16 5   UInt32 10   UInt64 20   Boolean 5
 *     Int8  4   Int16  6   Int32  11   Int64  20   Float32 48   Float64 327
 * Errors: data_capacity below the need is DFMI_ERR_CAPACITY (data_lengths set,
 * no byte of any column written); a column of 2^31 or more output bytes, or
 * 2^31 or more rows in the call, DFMI_ERR_NOT_IMPLEMENTED "device program
 * limit: ..."; a call without both flags DFMI_ERR_NOT_IMPLEMENTED; a Utf8
 * input, another type, a length that differs from num_rows[i] or a NULL buffer
 * DFMI_ERR_INVALID_ARGUMENT. Synchronous. The context keeps the call's scratch
 * (8 bytes per input row, rounded up to 256 rows per column, plus the scan's)
 * for later calls and frees it in dfmi_context_destroy: about 0.8 GB after a
 * call over 1e8 rows.
 * ------------------------------------------------------------------------- */
int32_t dfmi_format_utf8_batches(dfmi_context* ctx, const dfmi_column* columns, const int64_t* num_rows,
                                 int32_t num_columns, dfmi_out_column* outputs, int64_t* data_lengths,
                                 uint32_t flags, dfmi_error* err);

/* ---------------------------------------------------------------------------
 * CSV output (DFMI_FLAG_EXT_CSV_WRITE; the dialect is specified at the flag).
 *
 * dfmi_csv_header: the header line of `schema` into the HOST buffer `out`. Host
 * only: no context, no flag. *length is always written; capacity below it is
 * DFMI_ERR_CAPACITY with no byte written; out == NULL measures only. A NULL
 * schema, a schema without fields or a NULL name is DFMI_ERR_INVALID_ARGUMENT.
 *
 * dfmi_csv_encode_batches: `num_batches` device batches that share one
 * column-type list (0-row batches allowed, sliced columns through
 * dfmi_column.offset) as ONE byte stream of records in the device buffer
 * `data`, all columns of a row interleaved -- all the batches of a coalesced
 * pull in one call: the kernels run once over every batch together.
 *   *data_length   the bytes the call needs -- always written, also when the
 *                  call fails on a capacity or on the byte limit;
 *   batch_ends[i]  the bytes up to the end of batch i's last record (may be
 *                  NULL);
 *   measure mode   with data == NULL the call writes *data_length and
 *                  batch_ends and no byte. A caller whose schema holds Float64
 *                  or Utf8 columns measures, allocates exactly and calls again;
 *                  the others allocate rows * (the sum of the per-type worst
 *                  cases at dfmi_format_utf8_batches above + the column count).
 * Errors: data_capacity below the need is DFMI_ERR_CAPACITY (*data_length set,
 * no byte written); 2^31 or more rows in the call, 2^31 or more output bytes or
 * more than 256 columns DFMI_ERR_NOT_IMPLEMENTED "device program limit: ...";
 * a call without the flag DFMI_ERR_NOT_IMPLEMENTED; batches whose column types
 * differ, a type outside Boolean .. Utf8, a batch without columns, a length
 * that differs from num_rows or a NULL buffer DFMI_ERR_INVALID_ARGUMENT.
 * Synchronous. The context keeps the call's scratch (8 bytes per input row,
 * rounded up to 256 rows per batch, 4 more per row and Utf8 column, plus the
 * scan's) for later calls and frees it in dfmi_context_destroy.
 * ------------------------------------------------------------------------- */
int32_t dfmi_csv_header(const dfmi_schema* schema, uint8_t* out /* host */, int64_t capacity,
                        int64_t* length, dfmi_error* err);
int32_t dfmi_csv_encode_batches(dfmi_context* ctx, const dfmi_batch* inputs, int32_t num_batches,
                                uint8_t* data /* device; NULL: measure only */, int64_t data_capacity,
                                int64_t* data_length, int64_t* batch_ends /* [num_batches], may be NULL */,
                                uint32_t flags, dfmi_error* err);

/* ---------------------------------------------------------------------------
 * Multi-GPU. The reference is single-threaded (context.rs:33);
 * its pull is Relation::next (relation.rs:27-32). Rows are independent
 * through the Selection / Projection path and filter() keeps row order
 * (filter.rs:87-91), so a table shards by row range: one host thread or
 * process per GPU, each with its own context, calls the shard entry points
 * below on its own rows; per-rank outputs in rank order are the reference's
 * output stream. The only collective is one RCCL all_gather of a few int64
 * per rank after each pass (placement and errors); gathering results on one
 * rank is optional (grouped send/recv over xGMI).
 * ------------------------------------------------------------------------- */
#define DFMI_SHARD_ID_BYTES 128
typedef struct dfmi_shard_comm dfmi_shard_comm;

typedef struct dfmi_shard_placement {
    int32_t world, rank;
    int64_t row_offset;       /* first global output row of this rank's outputs */
    int64_t total_rows;       /* output rows over all ranks */
    int64_t utf8_base[16];    /* per output: global byte offset of this rank's Utf8 data */
    int64_t utf8_total[16];   /* per output: Utf8 bytes over all ranks */
    int64_t null_total[16];   /* per output: nulls over all ranks */
} dfmi_shard_placement;

/* A new RCCL unique id (rank 0), to be handed to every rank out of band. */
int32_t dfmi_shard_unique_id(uint8_t* id /* DFMI_SHARD_ID_BYTES */, dfmi_error* err);
/* Collective over `world` ranks (ncclCommInitRank on the context's device). */
int32_t dfmi_shard_comm_init(dfmi_context* ctx, int32_t world, int32_t rank, const uint8_t* id,
                             dfmi_shard_comm** out, dfmi_error* err);
void dfmi_shard_comm_destroy(dfmi_shard_comm* comm);
/* dfmi_filter_project over this rank's rows, then the placement exchange.
 * Collective: every rank calls it. When any rank fails, every rank returns
 * the error the reference would raise over the whole table (the smallest
 * evaluation position, then the earliest rows). */
int32_t dfmi_shard_filter_project(dfmi_context* ctx, dfmi_shard_comm* comm, const dfmi_program* predicate,
                                  const dfmi_program* const* projections, int32_t num_projections,
                                  const dfmi_batch* input, dfmi_out_column* outputs, uint32_t flags,
                                  dfmi_shard_placement* placement, dfmi_error* err);
/* Concatenate the last dfmi_shard_filter_project outputs on `root`, in rank
 * order (collective). `root_outputs` (root only) are device buffers sized for
 * placement.total_rows / utf8_total; Utf8 offsets are rebased, bitmaps
 * re-aligned. Fails (Capacity) if a gathered Utf8 column would pass 2^31 bytes. */
int32_t dfmi_shard_gather_to_root(dfmi_context* ctx, dfmi_shard_comm* comm, const dfmi_out_column* local_outputs,
                                  const dfmi_out_column* root_outputs, int32_t root, dfmi_error* err);
/* Aggregate extension across ranks (collective): every rank's exact partial
 * all_gathered and merged -- the values one GPU would produce over all rows. */
int32_t dfmi_shard_agg_finish(dfmi_context* ctx, dfmi_shard_comm* comm, dfmi_agg_state* state,
                              const dfmi_aggregate* const* aggs, int32_t num_aggs, dfmi_agg_value* out,
                              dfmi_error* err);
/* ... with a GROUP BY key (collective): every rank's per-group partials
 * all_gathered and merged; output as dfmi_agg_state_finish_grouped (every
 * rank gets the same groups; *num_groups set even past `capacity`). */
int32_t dfmi_shard_agg_finish_grouped(dfmi_context* ctx, dfmi_shard_comm* comm, dfmi_agg_state* state,
                                      const dfmi_aggregate* const* aggs, int32_t num_aggs, int64_t capacity,
                                      dfmi_agg_value* keys, dfmi_agg_value* values, int64_t* num_groups,
                                      dfmi_error* err);

#ifdef __cplusplus
}
#endif
#endif /* DFMI_H */
