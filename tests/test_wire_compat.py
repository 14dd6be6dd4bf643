"""Wire-compatibility check against the reference .proto schema.

tests/golden/wire_schema.json records every message field (NAME,
NUMBER, LABEL, type) and every rpc method name of the reference's proto
sources, parsed as text by tests/golden/regenerate.py. This test
verifies that every message field in our runtime-built descriptors
matches it. Field numbers + wire types are the wire contract; this test
is the automated proof that the schemas agree.
"""

import json
import os

from google.protobuf import descriptor_pool

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       'golden', 'wire_schema.json')

_SCALARS = {
    'double', 'float', 'int32', 'int64', 'uint32', 'uint64', 'sint32',
    'sint64', 'fixed32', 'fixed64', 'sfixed32', 'sfixed64', 'bool',
    'string', 'bytes',
}


def _golden() -> dict:
  with open(_GOLDEN) as f:
    return json.load(f)


def _reference_schema() -> dict:
  return _golden()['messages']


def test_every_reference_field_matches():
  import vizier_amd._src.service.proto.schema  # registers descriptors
  pool = descriptor_pool.Default()
  reference = _reference_schema()
  assert len(reference) > 30, 'parser failed to find reference messages'
  mismatches = []
  for full_name, fields in reference.items():
    try:
      desc = pool.FindMessageTypeByName(full_name)
    except KeyError:
      mismatches.append(f'missing message {full_name}')
      continue
    ours = {f.name: f for f in desc.fields}
    for fname, ref in fields.items():
      if fname not in ours:
        mismatches.append(f'{full_name}.{fname}: missing')
        continue
      f = ours[fname]
      if f.number != ref['number']:
        mismatches.append(
            f'{full_name}.{fname}: number {f.number} != {ref["number"]}')
      if f.is_repeated != ref['repeated']:
        mismatches.append(f'{full_name}.{fname}: repeated mismatch')
      ref_type = ref['type']
      if ref_type in _SCALARS:
        from google.protobuf import descriptor as _d
        expected = getattr(_d.FieldDescriptor,
                           'TYPE_' + ref_type.upper())
        if f.type != expected:
          mismatches.append(
              f'{full_name}.{fname}: scalar type {f.type} != {ref_type}')
      else:
        # Message or enum: compare the last name component.
        target = (f.message_type.name if f.message_type is not None
                  else f.enum_type.name if f.enum_type is not None
                  else None)
        if target != ref_type.split('.')[-1]:
          mismatches.append(
              f'{full_name}.{fname}: target {target} != {ref_type}')
  assert not mismatches, '\n'.join(mismatches)


def test_grpc_method_paths_match_reference_services():
  """Service + method names from the reference protos match our stubs."""
  from vizier_amd._src.service import service_stubs
  golden = _golden()
  assert golden['vizier_methods'] and golden['pythia_methods']
  assert set(golden['vizier_methods']) == set(service_stubs.VIZIER_METHODS)
  assert set(golden['pythia_methods']) == set(service_stubs.PYTHIA_METHODS)
