"""Regenerates the fixtures in this folder.

  python tests/golden/regenerate.py --upstream PATH [--gp-fit]

PATH is a checkout of the upstream OSS Vizier project (the directory
that holds `vizier/`). Two fixtures are read off it:

  wire_schema.json     every message field (name, number, label, type)
                       and every rpc method name in the upstream .proto
                       sources, parsed as text (no protoc needed);
                       compared with our runtime-built descriptors by
                       tests/test_wire_compat.py.
  public_exports.json  the names each upstream public module imports
                       into its namespace; tests/test_api_surface.py
                       requires ours to export them all.

--gp-fit also rewrites gp_posterior_n200_d10.json, the fitted raw GP
hyperparameters behind TestPosteriorScoreKernel in tests/test_gpu_ops.py.
The fp32 L-BFGS fit follows the CPU's reduction order (thread count,
vector width) to a different local optimum from machine to machine, so
the kernel-numerics tests pin one fit instead of refitting; leave it
alone unless the training data of that test changes.
"""

import argparse
import ast
import json
import os
import re
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
_TESTS = os.path.dirname(_HERE)
_REPO = os.path.dirname(_TESTS)

_PROTOS = ('key_value.proto', 'study.proto', 'vizier_oss.proto',
           'vizier_service.proto', 'pythia_service.proto')


def _strip_comments(text: str) -> str:
  # Line comments only: '/*' appears inside http-option path strings
  # (e.g. "owners/*/studies/*"), and upstream uses '//' throughout.
  return re.sub(r'//[^\n]*', '', text)


def _parse_block(text: str, start: int):
  """Returns (body, end) for the brace block starting at text[start]=='{'."""
  depth = 0
  for i in range(start, len(text)):
    if text[i] == '{':
      depth += 1
    elif text[i] == '}':
      depth -= 1
      if depth == 0:
        return text[start + 1:i], i + 1
  raise ValueError('Unbalanced braces')


_FIELD_RE = re.compile(
    r'(?P<label>optional\s+|repeated\s+)?'
    r'(?P<type>[\w.]+)\s+(?P<name>\w+)\s*=\s*(?P<number>\d+)')


def _parse_messages(text: str, prefix: str, out: dict):
  pos = 0
  while True:
    m = re.search(r'\b(message|enum)\s+(\w+)\s*{', text[pos:])
    if not m:
      break
    kind, name = m.group(1), m.group(2)
    body, endpos = _parse_block(text, pos + m.end() - 1)
    full = f'{prefix}.{name}'
    if kind == 'message':
      fields = {}
      # Remove nested blocks before scanning fields at this level.
      flat = ''
      i = 0
      while i < len(body):
        nested = re.search(r'\b(message|enum|oneof)\s+\w+\s*{', body[i:])
        if not nested:
          flat += body[i:]
          break
        flat += body[i:i + nested.start()]
        nested_body, nested_end = _parse_block(body,
                                               i + nested.end() - 1)
        if nested.group(1) == 'oneof':
          flat += nested_body  # oneof fields live at message level
        i = nested_end
      for fm in _FIELD_RE.finditer(flat):
        if fm.group('type') in ('option', 'reserved'):
          continue
        fields[fm.group('name')] = {
            'number': int(fm.group('number')),
            'type': fm.group('type'),
            'repeated': (fm.group('label') or '').strip() == 'repeated',
        }
      out[full] = fields
      _parse_messages(body, full, out)
    pos = endpos


def wire_schema(upstream: str) -> dict:
  service_dir = os.path.join(upstream, 'vizier', '_src', 'service')
  messages = {}
  texts = {}
  for fname in _PROTOS:
    with open(os.path.join(service_dir, fname)) as f:
      texts[fname] = _strip_comments(f.read())
    _parse_messages(texts[fname], 'vizier', messages)
  rpc = lambda fname: sorted(re.findall(r'rpc\s+(\w+)\s*\(', texts[fname]))
  return {
      'messages': messages,
      'vizier_methods': rpc('vizier_service.proto'),
      'pythia_methods': rpc('pythia_service.proto'),
  }


def public_exports(upstream: str) -> dict:
  sys.path.insert(0, _TESTS)
  sys.path.insert(0, _REPO)
  from test_api_surface import _MODULES
  out = {}
  for ref_path in sorted(_MODULES):
    with open(os.path.join(upstream, ref_path)) as f:
      tree = ast.parse(f.read())
    out[ref_path] = [a.asname or a.name for node in ast.walk(tree)
                     if isinstance(node, ast.ImportFrom)
                     for a in node.names]
  return out


def gp_fit() -> dict:
  sys.path.insert(0, _TESTS)
  sys.path.insert(0, _REPO)
  from test_gpu_ops import posterior_training_data
  from vizier_amd._src.gp import gp_model
  x, y = posterior_training_data()
  post = gp_model.train_gp(x, y, num_restarts=2, max_iters=20, seed=0)
  return {'raw': [float(v) for v in post.raw.float()], 'nll': post.nll}


def _write(name: str, obj) -> None:
  with open(os.path.join(_HERE, name), 'w') as f:
    json.dump(obj, f, indent=1, sort_keys=True)
    f.write('\n')
  print('wrote', name)


def main() -> None:
  parser = argparse.ArgumentParser()
  parser.add_argument('--upstream', default=None)
  parser.add_argument('--gp-fit', action='store_true')
  args = parser.parse_args()
  if args.upstream:
    _write('wire_schema.json', wire_schema(args.upstream))
    _write('public_exports.json', public_exports(args.upstream))
  if args.gp_fit:
    _write('gp_posterior_n200_d10.json', gp_fit())


if __name__ == '__main__':
  main()
