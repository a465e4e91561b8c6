"""Records the flags of the reference's TrainArgParser into train_cli_flags.json (settings only):

    python tests/golden/make_train_cli_flags.py REFERENCE_DIR

REFERENCE_DIR holds the reference's args.py, which needs argparse and numpy alone.  For every option action of its parser:
flag, dest, type (by name), default, choices, required and whether it is a store_true switch.  tests/test_train_cli_host.py
holds `bts_amd.train.arg_parser()` against the file."""
import json
import os
import sys


def record(parser):
    flags = []
    for a in parser._actions:
        if not a.option_strings or a.dest == 'help':
            continue
        flags.append({'flag': a.option_strings[0], 'dest': a.dest, 'type': a.type.__name__ if a.type is not None else None,
                      'default': a.default, 'choices': list(a.choices) if a.choices is not None else None,
                      'required': bool(a.required), 'store_true': a.nargs == 0 and a.const is True})
    return flags


def main(argv):
    sys.path.insert(0, os.path.abspath(argv[1]))
    import args as reference_args
    flags = record(reference_args.TrainArgParser().parser)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'train_cli_flags.json')
    with open(out, 'w') as f:
        json.dump({'parser': 'TrainArgParser', 'flags': flags}, f, indent=1)
        f.write('\n')
    print('%d flags -> %s' % (len(flags), out))


if __name__ == '__main__':
    main(sys.argv)
