/* cliopt_driver.c -- a stand-alone program over host/cliopt.c: a table with one
 * row of every kind, parsed from argv and printed.  tests/test_cliopt_driver.py
 * builds it with -fsanitize=address,undefined and runs it on the host.
 *   cliopt_driver s|l [words...]   s: one trailing input, a bare `--` skipped
 *                                  l: trailing words are a list, `--` unknown */
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "cliopt.h"

typedef struct {
	int flag, num, pick;
	unsigned udbl;
	const char *str, *unset, *unsup, *rest;
	char ch;
	double dbl, pct;
	cli_prec prec;
	cli_list list, need;
} Opts;

#define F(f) offsetof(Opts, f)
static const cli_name picks[] = {{"one", 1}, {"two", 2}, {NULL, 0}};
static const cli_opt rows[] = {
	{'p', "flag", CLI_FLAG, F(flag), 4, "a flag", "0"},
	{'U', "unset", CLI_UNSET, F(unset), 0, "a string to NULL", ""},
	{'g', "ignore", CLI_IGNORE, 0, 0, "ignored", ""},
	{'G', "ignore_end", CLI_IGNORE, 0, 0, "ignored, ends its word", "", CLI_ENDS_WORD},
	{'h', "help", CLI_HELP, 0, 0, "this table", ""},
	{'o', "str", CLI_STR, F(str), 0, "a string", "-"},
	{'S', "char", CLI_CHAR, F(ch), 0, "a character", "\\t"},
	{'x', "int", CLI_INT, F(num), 0, "a checked integer", "9"},
	{'e', "dbl", CLI_DBL, F(dbl), 0, "a checked double", "10.0"},
	{'C', "pct", CLI_PCT, F(pct), 0, "a percentage", "50.0%"},
	{'E', "udbl", CLI_UDBL, F(udbl), 0, "an unsigned through strtod", "15"},
	{'s', "prec", CLI_PREC, F(prec), 2, "a mark and an optional number", "1e0"},
	{'T', "drop", CLI_DROP, 0, 0, "dropped", ""},
	{'t', "drop_int", CLI_DROP, 0, 1, "checked, then dropped", "1"},
	{'a', "unsup", CLI_UNSUP, F(unsup)},
	{0, "pick", CLI_ENUM, F(pick), 0, "one / two", "one", 0, picks},
	{'i', "list", CLI_LIST, F(list), 0, "a file list", "stdin"},
	{'I', "need", CLI_LIST, F(need), 0, "a file list of at least one", "stdin", CLI_NEEDS_ONE},
	{0}};
static const cli_cmd single = {"#driver: one input", rows, "Unknown argument:\t\"%s\"\n",
                               "Unexpected non-option argument(s).\n", 1, 0, F(rest)};
static const cli_cmd listed = {"#driver: a list of inputs", rows, "Unknown argument or option: \"%s\"\n", NULL, 0, 1, F(list)};
#undef F

static void print_list(const char *what, const cli_list *L) {
	printf("%s=%d", what, L->n);
	for(int i = 0; i < L->n; ++i) printf(" [%s]", L->v[i]);
	printf("\n");
}

int main(int argc, char **argv) {
	Opts o = {.num = 9, .pick = 1, .udbl = 15, .str = "-", .unset = "set", .rest = "-", .ch = '\t', .dbl = 10.0,
	          .pct = 0.5, .prec = {8, 1.0}};
	if(argc < 2 || (strcmp(argv[1], "s") && strcmp(argv[1], "l"))) return 2;
	const int rc = cli_parse(argv[1][0] == 's' ? &single : &listed, argc - 1, argv + 1, &o);
	if(rc != CLI_GO) return rc;
	printf("flag=%d num=%d pick=%d udbl=%u ch=%d dbl=%g pct=%g prec=%d/%g\n", o.flag, o.num, o.pick, o.udbl, o.ch,
	       o.dbl, o.pct, o.prec.mark, o.prec.scale);
	printf("str=[%s] unset=[%s] unsup=[%s] rest=[%s]\n", o.str, o.unset ? o.unset : "(null)",
	       o.unsup ? o.unsup : "(null)", o.rest);
	print_list("list", &o.list);
	print_list("need", &o.need);
	return 0;
}
