/*
 * cliopt.h -- one option table per command, parsed and printed by one walker.
 *
 * A command declares a struct of its options (defaults in the initialiser), a
 * `static const cli_opt[]` whose rows stand in help order, and a cli_cmd with
 * what differs between commands (banner, message formats, how trailing words
 * are taken).  cli_parse walks argv once and stores into the struct; `-h`
 * prints the same table.  stdio, stdlib and string only.
 */
#ifndef CCPHYLO_CLIOPT_H
#define CCPHYLO_CLIOPT_H
#include <stddef.h>
#include <stdio.h>

enum cli_kind {
	CLI_FLAG,    /* int field = konst                                        no value */
	CLI_UNSET,   /* string field = NULL (the `-M` / `-D` sub-help marks)     no value */
	CLI_IGNORE,  /* accepted, no effect                                      no value */
	CLI_HELP,    /* prints the table to stdout, ends the run with status 0 */
	CLI_STR,     /* const char * field = the value */
	CLI_CHAR,    /* char field = the value's first character */
	CLI_INT,     /* int / unsigned field = strtol of the whole value, else "Invalid" */
	CLI_DBL,     /* double field = strtod of the whole value, else "Invalid" */
	CLI_PCT,     /* double field = strtod(value) / 100, unchecked */
	CLI_UDBL,    /* unsigned field = (unsigned) strtod(value), unchecked */
	CLI_PREC,    /* cli_prec field: mark = konst; scale = the next word if it is given
	                and does not start with '-' (a number, else "Invalid") */
	CLI_DROP,    /* value taken and dropped; konst 1: checked as CLI_INT first */
	CLI_UNSUP,   /* value taken and dropped; const char * field = the option as typed */
	CLI_ENUM,    /* int field = id of the value in `names`, else "Invalid" */
	CLI_LIST     /* cli_list field: the attached value or the next word, then every
	                following word that is no option */
};

typedef struct {
	const char *name;   /* NULL ends a table */
	int id;
} cli_name;

typedef struct {
	int mark;
	double scale;
} cli_prec;

typedef struct {
	char **v;   /* points into argv */
	int n;
} cli_list;

/* cli_opt.bits: a command's oddities, kept as data */
#define CLI_ENDS_WORD 1   /* a no-value option after which the rest of a short-option word is dropped */
#define CLI_NEEDS_ONE 2   /* a CLI_LIST without a first value is "Missing" (named by its long name) */

typedef struct {
	char letter;             /* 0: long form only */
	const char *name;        /* long name; NULL ends the table */
	int kind;
	size_t off;              /* offsetof the field in the command's struct */
	int konst;
	const char *desc, *def;  /* help columns; desc NULL: parsed, not listed */
	int bits;
	const cli_name *names;   /* CLI_ENUM */
} cli_opt;

typedef struct {
	const char *banner;       /* first help line */
	const cli_opt *opts;
	const char *unknown_fmt;  /* one %s: the option as typed */
	const char *extra_msg;    /* a second trailing word, where the command takes one input */
	int skip_dashdash;        /* a bare `--` is skipped, not unknown */
	int rest_list;            /* trailing words: 1 a cli_list at rest_off, 0 one const char * */
	size_t rest_off;
} cli_cmd;

#define CLI_GO (-1)

/* CLI_GO, or the exit status the command ends with (help 0, a fault 1 after its message) */
int cli_parse(const cli_cmd *cmd, int argc, char **argv, void *opts);
void cli_help(const cli_cmd *cmd, FILE *out);

#endif
