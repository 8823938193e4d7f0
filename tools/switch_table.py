"""Prints the README's switch table (markdown) from the two switch tables: the native library's (csrc/switches.h, through
mmnas_switch_info -- the library must be built) and mmnas_amd/switches.py.  README.md holds the output between
`<!-- switch-table:begin -->` and `<!-- switch-table:end -->`; tests/test_switches_host.py compares the two.

    python tools/switch_table.py            # print
    python tools/switch_table.py --write    # replace the section of README.md
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BEGIN, END = '<!-- switch-table:begin -->', '<!-- switch-table:end -->'


def table():
    from mmnas_amd import switches as S
    rows = {}
    for name, r in S.native().items():
        kind, policy, text = re.match(r'\[(\w+), (\w+)\] (.*)', r['help']).groups()
        dflt = '—' if kind in ('string', 'presence') else str(r['default'])
        rows[name] = [name, 'native', dflt, kind, policy, text]
    for name, f in S.TABLE.items():
        dflt = '—' if f.default is None or f.kind == 'presence' else str(int(f.default))
        if name in rows:   # read on both sides: one row, both descriptions
            if f.policy != 'doc':
                rows[name][1] = 'both'
                rows[name][5] += ' / Python (%s, %s): %s' % (f.kind, f.policy, f.help)
        else:
            rows[name] = [name, 'python', dflt, f.kind, f.policy, f.help]
    out = ['| variable | side | default | kind | read | effect |', '|---|---|---|---|---|---|']
    for name in sorted(rows):
        r = rows[name]
        out.append('| `%s` | %s | %s | %s | %s | %s |' % (r[0], r[1], r[2], r[3], r[4], r[5].replace('|', '\\|')))
    return '\n'.join(out)


def readme_section(text):
    return text[text.index(BEGIN) + len(BEGIN):text.index(END)].strip('\n')


if __name__ == '__main__':
    t = table()
    if '--write' in sys.argv[1:]:
        path = os.path.join(ROOT, 'README.md')
        text = open(path).read()
        a, b = text.index(BEGIN) + len(BEGIN), text.index(END)
        open(path, 'w').write(text[:a] + '\n' + t + '\n' + text[b:])
    else:
        print(t)
