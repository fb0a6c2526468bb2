/* cliopt.c -- the option walker of the command line (cliopt.h) */
#include <stdlib.h>
#include <string.h>
#include "cliopt.h"

typedef struct {
	int argc, k;
	char **argv;
} Walk;

static int fault(const char *kind, const char *opt) {
	fprintf(stderr, "%s argument:\t\"%s\"\n", kind, opt);
	return 1;
}

/* value of an option: attached ("-x5", "--opt=5") or the next argv word; NULL when there is none */
static char *value(Walk *W, char *att) {
	if(att && *att) return att;
	if(W->k + 1 < W->argc) return W->argv[++W->k];
	return NULL;
}

static int is_option(const char *a) {
	return a[0] == '-' && a[1] != 0;
}

/* stores one option; CLI_GO or the status to end with.  `typed` is the name in messages */
static int apply(const cli_cmd *cmd, const cli_opt *o, Walk *W, char *att, const char *typed, void *opts) {
	void *field = (char *) opts + o->off;
	char *v = NULL, *e;
	switch(o->kind) {
		case CLI_FLAG: *(int *) field = o->konst; return CLI_GO;
		case CLI_UNSET: *(const char **) field = NULL; return CLI_GO;
		case CLI_IGNORE: return CLI_GO;
		case CLI_HELP: cli_help(cmd, stdout); return 0;
		case CLI_PREC:   /* cmdline.c getdDefArg: the value is optional */
			((cli_prec *) field)->mark = o->konst;
			if(att && *att) v = att;
			else if(W->k + 1 < W->argc && W->argv[W->k + 1][0] != '-') v = W->argv[++W->k];
			if(!v) return CLI_GO;
			((cli_prec *) field)->scale = strtod(v, &e);
			return (!*v || *e) ? fault("Invalid", typed) : CLI_GO;
		case CLI_LIST: {
			cli_list *L = field;
			if(o->bits & CLI_NEEDS_ONE) {
				if(!(v = value(W, att))) return fault("Missing", o->name);
			} else {
				v = att;
			}
			if(v) W->argv[W->k] = v;
			L->v = W->argv + W->k + (v ? 0 : 1);
			L->n = v ? 1 : 0;
			for(; W->k + 1 < W->argc && !is_option(W->argv[W->k + 1]); ++W->k) ++L->n;
			return CLI_GO;
		}
		default: break;
	}
	if(!(v = value(W, att))) return fault("Missing", typed);
	switch(o->kind) {
		case CLI_STR: *(const char **) field = v; break;
		case CLI_CHAR: *(char *) field = v[0]; break;
		case CLI_INT:
		case CLI_DROP: {
			if(o->kind == CLI_DROP && !o->konst) break;
			const long x = strtol(v, &e, 10);
			if(*e) return fault("Invalid", typed);
			if(o->kind == CLI_INT) *(int *) field = (int) x;
			break;
		}
		case CLI_DBL:
			*(double *) field = strtod(v, &e);
			if(*e) return fault("Invalid", typed);
			break;
		case CLI_PCT: *(double *) field = strtod(v, NULL) / 100; break;
		case CLI_UDBL: *(unsigned *) field = (unsigned) strtod(v, NULL); break;
		case CLI_UNSUP: *(const char **) field = typed; break;
		case CLI_ENUM: {
			const cli_name *t = o->names;
			while(t->name && strcmp(t->name, v)) ++t;
			if(!t->name) {
				fprintf(stderr, "Invalid argument:\t\"\"--%s\"\"\n", o->name);
				return 1;
			}
			*(int *) field = t->id;
			break;
		}
	}
	return CLI_GO;
}

static int takes_value(const cli_opt *o) {
	return o->kind >= CLI_STR || (o->bits & CLI_ENDS_WORD);
}

static int unknown(const cli_cmd *cmd, const char *typed) {
	fprintf(stderr, cmd->unknown_fmt, typed);
	return 1;
}

int cli_parse(const cli_cmd *cmd, int argc, char **argv, void *opts) {
	static char letter[2];   /* a short option as typed; static: CLI_UNSUP keeps it */
	Walk W = {argc, 0, argv};
	for(W.k = 1; W.k < argc; ++W.k) {
		char *a = argv[W.k];
		const cli_opt *o = cmd->opts;
		int rc;
		if(!is_option(a)) {   /* the input(s), and the end of the options */
			if(cmd->rest_list) {
				cli_list *L = (cli_list *) ((char *) opts + cmd->rest_off);
				L->v = argv + W.k;
				L->n = argc - W.k;
			} else {
				*(const char **) ((char *) opts + cmd->rest_off) = a;
				if(W.k + 1 < argc) {
					fputs(cmd->extra_msg, stderr);
					return 1;
				}
			}
			break;
		}
		if(a[1] == '-') {
			char *name = a + 2, *eq = strchr(name, '='), *att = NULL;
			if(eq) {
				*eq = 0;
				att = eq + 1;
			}
			if(*name == 0 && cmd->skip_dashdash) continue;
			while(o->name && strcmp(o->name, name)) ++o;
			if(!o->name) return unknown(cmd, a);
			if((rc = apply(cmd, o, &W, att, name, opts)) != CLI_GO) return rc;
			continue;
		}
		for(char *p = a + 1; *p; ++p) {
			char bad[3] = {'-', *p, 0};
			for(o = cmd->opts; o->name && o->letter != *p; ++o) { }
			if(!o->name) return unknown(cmd, bad);
			letter[0] = *p;
			if((rc = apply(cmd, o, &W, p[1] ? p + 1 : NULL, letter, opts)) != CLI_GO) return rc;
			if(takes_value(o)) break;
		}
	}
	return CLI_GO;
}

void cli_help(const cli_cmd *cmd, FILE *out) {
	fprintf(out, "%s\n", cmd->banner);
	fprintf(out, "#   %-24s\t%-32s\t%s\n", "Options are:", "Desc:", "Default:");
	for(const cli_opt *o = cmd->opts; o->name; ++o) {
		if(!o->desc) continue;
		if(o->letter) fprintf(out, "#    -%c, --%-16s\t%-32s\t%s\n", o->letter, o->name, o->desc, o->def);
		else fprintf(out, "#        --%-16s\t%-32s\t%s\n", o->name, o->desc, o->def);
	}
}
